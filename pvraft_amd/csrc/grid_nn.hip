// K25: nearest support point within a radius on a hashed cell grid, and the
// point-to-point ICP refinement built on it (both absent in the reference).
//
//   Search.  inv = fp32(1) / fp32(radius) and r2 = fp32(radius)^2 come from the
//   host.  With R, t (read from DEVICE memory) the query point is first mapped,
//   x' = ((R00*x + R01*y) + R02*z) + t0 and likewise y', z', every operation an
//   fp32 operation rounded on its own (fp contract off for this file).
//   q = floor(fp32(x * inv)) per coordinate.  Eligible: masked, finite,
//   -2^20 <= q < 2^20 on all three axes (nf_cell's rules), cell c = int(q); a
//   query by the same rules on the mapped point.
//   j is a candidate of query i: j an eligible support point of the same batch
//   element, max|c_i - c_j| <= 1 and d2 = (dx*dx + dy*dy) + dz*dz <= r2 in
//   fp32, dx = x'_i - x_j.  idx_i = the candidate with the smallest d2, ties to
//   the smallest j; no candidate or an ineligible query: idx = -1, d2 = +INF.
//   out: idx (B,Nq) int32, d2 (B,Nq), ok (B) bool.
//
// 6 launches.  Kernel boundaries are the only global synchronisation; no lane
// or workgroup ever waits for another one's progress.  All atomics are integer
// (compare-and-swap, add).  The order in which they land decides only the
// order of the points inside a cell of the sorted array, and the query
// compares (d2, original index), so no output depends on it.
//
//  1. gn_init_kernel     table keys = empty word, cell counters = 0, the int
//                        state words = 0, ok = 1; for ICP also (R, t) = (R0,
//                        t0) or the identity.  Every workspace word that is
//                        read later is written here or by a later kernel
//                        before its use.
//  2. gn_count_kernel    one lane per support point: eligibility, the 63-bit
//                        cell key, find-or-claim of the key's slot in a table
//                        of T >= 2 M slots (a power of two) per cloud, ONE
//                        compare-and-swap per probe step, capped at T steps
//                        (status[b] = 1, ok[b] = 0 at the cap), add 1 to the
//                        cell counter, remember the slot.
//  3. gn_scan_kernel     exclusive scan of the counters inside every run of
//                        GN_THREADS slots, the run totals to bsum.
//  4. gn_offset_kernel   one wave per cloud: exclusive scan of bsum.
//  5. gn_scatter_kernel  one integer add per point on its cell's cursor, then
//                        (x, y, z, index) into the cell-sorted array.
//  6. gn_query_kernel    one lane per query: map, cell, 27 finds (plain loads:
//                        the table is final), 16-byte loads of the sorted
//                        records, the running best (d2, index, and for ICP the
//                        point) in registers, GN_UNROLL records in flight
//                        per lane (one at a time was a chain of memory
//                        latencies: 3.6 ms instead of 1.8 ms at 131072 x
//                        131072).  Queries are not sorted by cell, so the
//                        lanes of a wave walk different cells; the trace puts
//                        the time in the densest cells (the slowest lane),
//                        not in that divergence, so sorting them first was
//                        NOT built.  The table holds
//                        at most M < T keys, so a probe meets an empty slot
//                        within M + 1 steps and cannot reach its cap; the loop
//                        bound stays as a guard (that query then reports -1
//                        and ok[b] = 0).  With status[b] set by launch 2 every
//                        idx of the cloud is -1.
//
// These are the grid steps of noise_filter.hip written a second time (gn_
// names): that file is untouched, so its outputs stay bit-identical by
// construction.  A change to the cell rules belongs in both.
//
// ICP (ops.icp_refine): launches 1-5 once over dst, then per round
//   a. gn_query_kernel<true>   the search under the current (R, t), which also
//                              writes the matched point (src itself without a
//                              match), the Cauchy weight w = 1 / (1 + d2 / th2)
//                              (0 without a match; th2 = fp32(thresh)^2 from
//                              the host, both divisions correctly rounded) and
//                              adds the number of matches to the round's
//                              counter, one integer add per wave;
//   b. rigid_fit_kernel        (rigid_fit.hip, iters = 0) of src against the
//                              matched points with those weights, into
//                              scratch (R, t);
//   c. gn_commit_kernel        one lane per cloud: not stopped, >= 3 matches
//                              and the fit ok -> (R, t) = the fit, rounds += 1;
//                              otherwise stopped = 1, ok = 0 and (R, t) stay.
// and one closing gn_query_kernel<true> whose counter is `matched`:
// 5 + 3 * iters + 1 launches, fixed by iters; (R, t), stopped and the counters
// live in device memory, no host synchronisation.  A stopped cloud still runs
// its searches (under an unchanged (R, t) they repeat themselves).  The fit is
// the existing one-launch kernel on purpose: it has the documented semantics of
// ops.rigid_fit(iters=0) by being that code.  The alternative (per-workgroup
// fp64 partial sums in the query kernel, folded in a fixed order, plus the 3x3
// solve) would save the (B,N,3) + (B,N) round trip and one launch per round.
// Traced on an MI355X the fit is 31.5 us per round, 12 % of an ICP call at 8192
// x 8192 points and 1.2 % at 8192 x 131072 (profiles/README.md): that is the
// most the alternative could save, so it was NOT built.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), VGPRs /
// LDS bytes / scratch bytes: init 14 / 0 / 0, count 12 / 0 / 0, scan 10 / 16 /
// 0, offset 14 / 0 / 0, scatter 8 / 0 / 0, query<false> 49 / 0 / 0,
// query<true> 60 / 0 / 0, commit 23 / 0 / 0; no AGPRs, 8 waves per SIMD
// everywhere.
#include <hip/hip_runtime.h>
#include "common.h"

#pragma clang fp contract(off)

#define GN_THREADS 256
#define GN_WAVES (GN_THREADS / WAVE)
#define GN_SCAN 64  // lanes of the run-total scan: one wave
#define GN_RANGE (1 << 20)
#define GN_EMPTY (~0ull)  // no key has bit 63 set
#define GN_UNROLL 8  // sorted records in flight per lane in the query's member loop

typedef unsigned long long gn_u64;

int grid_nn_block() { return GN_THREADS; }

// slot hash: the 64-bit finaliser of noise_filter.hip / voxel_sample.hip
DEV_INLINE unsigned gn_slot_hash(gn_u64 k) {
  k ^= k >> 33;
  k *= 0xFF51AFD7ED558CCDull;
  k ^= k >> 33;
  k *= 0xC4CEB9FE1A85EC53ull;
  k ^= k >> 33;
  return (unsigned)k;
}

DEV_INLINE gn_u64 gn_key(int cx, int cy, int cz) {
  return ((gn_u64)(cx + GN_RANGE) << 42) | ((gn_u64)(cy + GN_RANGE) << 21) | (gn_u64)(cz + GN_RANGE);
}

// Cell of a point; false if the point is not eligible (the mask aside).
DEV_INLINE bool gn_cell(float x, float y, float z, float inv, int &cx, int &cy, int &cz) {
  const float qx = floorf(x * inv), qy = floorf(y * inv), qz = floorf(z * inv);
  const float lo = -(float)GN_RANGE, hi = (float)GN_RANGE;
  const bool el = isfinite(x) && isfinite(y) && isfinite(z) && qx >= lo && qx < hi && qy >= lo &&
                  qy < hi && qz >= lo && qz < hi;
  cx = el ? (int)qx : 0;
  cy = el ? (int)qy : 0;
  cz = el ? (int)qz : 0;
  return el;
}

// Finds or claims the slot of `key`; -1 at the cap.
DEV_INLINE int gn_insert(gn_u64 *keys, int T, gn_u64 key) {
  unsigned s = gn_slot_hash(key) & (unsigned)(T - 1);
  for (int step = 0; step < T; ++step) {
    gn_u64 seen = GN_EMPTY;
    const bool claimed = __hip_atomic_compare_exchange_strong(
        keys + s, &seen, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (claimed || seen == key) return (int)s;
    s = (s + 1u) & (unsigned)(T - 1);
  }
  return -1;
}

// Slot of `key` in the finished table, -1 if the cell is empty, -2 at the cap.
DEV_INLINE int gn_find(const gn_u64 *__restrict__ keys, int T, gn_u64 key) {
  unsigned s = gn_slot_hash(key) & (unsigned)(T - 1);
  for (int step = 0; step < T; ++step) {
    const gn_u64 seen = keys[s];
    if (seen == key) return (int)s;
    if (seen == GN_EMPTY) return -1;
    s = (s + 1u) & (unsigned)(T - 1);
  }
  return -2;
}

// state: nstate ints, all zeroed (status (B) first).  Rcur / tcur: null for the
// plain search; R0 / t0 null: identity / zero.
__global__ __launch_bounds__(GN_THREADS) void gn_init_kernel(
    gn_u64 *__restrict__ keys, int *__restrict__ cnt, long slots, int *__restrict__ state,
    long nstate, unsigned char *__restrict__ ok, float *__restrict__ Rcur,
    float *__restrict__ tcur, const float *__restrict__ R0, const float *__restrict__ t0, int B) {
  const long t = (long)blockIdx.x * GN_THREADS + threadIdx.x;
  const long stride = (long)gridDim.x * GN_THREADS;
  for (long j = t; j < slots; j += stride) {
    keys[j] = GN_EMPTY;
    cnt[j] = 0;
  }
  for (long j = t; j < nstate; j += stride) state[j] = 0;
  for (long j = t; j < B; j += stride) ok[j] = 1;
  if (Rcur != nullptr) {
    for (long j = t; j < (long)B * 9; j += stride)
      Rcur[j] = R0 != nullptr ? R0[j] : ((j % 9) % 4 == 0 ? 1.0f : 0.0f);
    for (long j = t; j < (long)B * 3; j += stride) tcur[j] = t0 != nullptr ? t0[j] : 0.0f;
  }
}

__global__ __launch_bounds__(GN_THREADS) void gn_count_kernel(
    const float *__restrict__ xyz,           // (B, M, 3)
    const unsigned char *__restrict__ mask,  // (B, M) or null
    gn_u64 *keys, int *cnt,                  // (B, T) each
    int *__restrict__ slot,                  // (B, M)
    int *status, unsigned char *ok, int M, int T, float inv) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * GN_THREADS + threadIdx.x;
  if (i >= M) return;
  const long g = (long)b * M + i;
  int cx, cy, cz;
  const bool el = gn_cell(xyz[g * 3 + 0], xyz[g * 3 + 1], xyz[g * 3 + 2], inv, cx, cy, cz) &&
                  (mask == nullptr || mask[g] != 0);
  int s = -1;
  if (el) {
    s = gn_insert(keys + (long)b * T, T, gn_key(cx, cy, cz));
    if (s < 0) {
      __hip_atomic_store(status + b, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      ok[b] = 0;
    } else {
      atomicAdd(cnt + (long)b * T + s, 1);
    }
  }
  slot[g] = s;
}

// Exclusive prefix of v over the workgroup's GN_THREADS lanes.
DEV_INLINE int gn_block_excl(int v, int *wsum) {
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
  for (int w = 0; w < GN_WAVES; ++w) base += w < wave_id() ? wsum[w] : 0;
  return base + x - v;
}

__global__ __launch_bounds__(GN_THREADS) void gn_scan_kernel(
    const int *__restrict__ cnt, int *__restrict__ cur, int *__restrict__ bsum, int T) {
  __shared__ int wsum[GN_WAVES];
  const int b = blockIdx.y;
  const int s = blockIdx.x * GN_THREADS + threadIdx.x;
  const int v = s < T ? cnt[(long)b * T + s] : 0;
  const int ex = gn_block_excl(v, wsum);
  if (s < T) cur[(long)b * T + s] = ex;
  if (threadIdx.x == GN_THREADS - 1) bsum[(long)b * gridDim.x + blockIdx.x] = ex + v;
}

__global__ __launch_bounds__(GN_SCAN) void gn_offset_kernel(int *__restrict__ bsum, int nrun) {
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  bsum += (long)b * nrun;
  int run = 0;
  for (int base = 0; base < nrun; base += GN_SCAN) {
    const int j = base + lane;
    const int v = j < nrun ? bsum[j] : 0;
    int x = v;
#pragma unroll
    for (int off = 1; off < GN_SCAN; off <<= 1) {
      const int y = __shfl_up(x, off, WAVE);
      if (lane >= off) x += y;
    }
    if (j < nrun) bsum[j] = run + x - v;
    run += __shfl(x, GN_SCAN - 1, WAVE);
  }
}

__global__ __launch_bounds__(GN_THREADS) void gn_scatter_kernel(
    const float *__restrict__ xyz, const int *__restrict__ slot, int *cur,
    const int *__restrict__ bsum, float4 *__restrict__ sorted, int M, int T, int nrun) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * GN_THREADS + threadIdx.x;
  if (i >= M) return;
  const long g = (long)b * M + i;
  const int s = slot[g];
  if (s < 0) return;
  const int pos = bsum[(long)b * nrun + s / GN_THREADS] + atomicAdd(cur + (long)b * T + s, 1);
  if (pos >= 0 && pos < M)  // holds by construction: the counters sum to at most M
    sorted[(long)b * M + pos] =
        make_float4(xyz[g * 3 + 0], xyz[g * 3 + 1], xyz[g * 3 + 2], __int_as_float(i));
}

// ICP = false: the plain search (mdst, wgt, matched unused).  R / t: null or
// (B, 3, 3) / (B, 3) in device memory.
template <bool ICP>
__global__ __launch_bounds__(GN_THREADS) void gn_query_kernel(
    const float *__restrict__ query,          // (B, Nq, 3)
    const unsigned char *__restrict__ qmask,  // (B, Nq) or null
    const float *__restrict__ R, const float *__restrict__ t,
    const float4 *__restrict__ sorted, const gn_u64 *__restrict__ keys,
    const int *__restrict__ cnt, const int *__restrict__ cur, const int *__restrict__ bsum,
    const int *__restrict__ status, unsigned char *ok, int *__restrict__ idx_out,
    float *__restrict__ d2_out, float *__restrict__ mdst, float *__restrict__ wgt, int *matched,
    int Nq, int M, int T, int nrun, float inv, float r2, float th2) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * GN_THREADS + threadIdx.x;
  const bool live = i < Nq;
  const long g = (long)b * Nq + (live ? i : 0);
  sorted += (long)b * M;
  keys += (long)b * T;
  cnt += (long)b * T;
  cur += (long)b * T;
  bsum += (long)b * nrun;
  const float sx = query[g * 3 + 0], sy = query[g * 3 + 1], sz = query[g * 3 + 2];
  float x = sx, y = sy, z = sz;
  if (R != nullptr) {
    const float *Rb = R + (long)b * 9, *tb = t + (long)b * 3;
    x = ((Rb[0] * sx + Rb[1] * sy) + Rb[2] * sz) + tb[0];
    y = ((Rb[3] * sx + Rb[4] * sy) + Rb[5] * sz) + tb[1];
    z = ((Rb[6] * sx + Rb[7] * sy) + Rb[8] * sz) + tb[2];
  }
  int cx = 0, cy = 0, cz = 0;
  const bool el = live && gn_cell(x, y, z, inv, cx, cy, cz) &&
                  (qmask == nullptr || qmask[g] != 0) && status[b] == 0;
  float best = INFINITY;
  int bi = -1;
  float bx = sx, by = sy, bz = sz;
  bool capped = false;
  if (el) {
    for (int c = 0; c < 27; ++c) {
      const int nx = cx + c / 9 - 1, ny = cy + (c / 3) % 3 - 1, nz = cz + c % 3 - 1;
      if (nx < -GN_RANGE || nx >= GN_RANGE || ny < -GN_RANGE || ny >= GN_RANGE || nz < -GN_RANGE ||
          nz >= GN_RANGE)
        continue;  // no eligible point has such a cell
      const int s = gn_find(keys, T, gn_key(nx, ny, nz));
      if (s < 0) {
        capped = capped || s == -2;
        continue;
      }
      int end = bsum[s / GN_THREADS] + cur[s];
      if (end > M) end = M;
      int j = end - cnt[s];
      if (j < 0) j = 0;
      auto visit = [&](const float4 o) __attribute__((always_inline)) {
        const float dx = x - o.x, dy = y - o.y, dz = z - o.z;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        const int oi = __float_as_int(o.w);
        if (d2 <= r2 && (d2 < best || (d2 == best && (bi < 0 || oi < bi)))) {
          best = d2;
          bi = oi;
          if (ICP) {
            bx = o.x;
            by = o.y;
            bz = o.z;
          }
        }
      };
      // GN_UNROLL records (one 128-byte line) are loaded before the first is
      // used: a dense cell is a walk over consecutive records, and one load
      // at a time makes it a chain of memory latencies.  The comparison is on
      // (d2, original index), so the order of the visits does not matter.
      for (; j + GN_UNROLL <= end; j += GN_UNROLL) {
        float4 o[GN_UNROLL];
#pragma unroll
        for (int u = 0; u < GN_UNROLL; ++u) o[u] = sorted[j + u];
#pragma unroll
        for (int u = 0; u < GN_UNROLL; ++u) visit(o[u]);
      }
      for (; j < end; ++j) visit(sorted[j]);
    }
  }
  if (capped) {  // unreachable with T >= 2 M, see the header
    ok[b] = 0;
    best = INFINITY;
    bi = -1;
    bx = sx, by = sy, bz = sz;
  }
  const bool found = live && bi >= 0;
  if (live) {
    idx_out[g] = bi;
    d2_out[g] = best;
  }
  if (ICP) {
    if (live) {
      mdst[g * 3 + 0] = bx;
      mdst[g * 3 + 1] = by;
      mdst[g * 3 + 2] = bz;
      // 1 / (1 + d2 / th2): both divisions are the correctly rounded sequences
      wgt[g] = found ? 1.0f / (1.0f + best / th2) : 0.0f;
    }
    const int n = __popcll(__ballot(found));
    if (lane_id() == 0 && n > 0) atomicAdd(matched + b, n);
  }
}

// One lane per cloud.  cnt: the matches of this round's search.
__global__ __launch_bounds__(GN_THREADS) void gn_commit_kernel(
    const int *__restrict__ cnt, const unsigned char *__restrict__ fit_ok,
    const float *__restrict__ Rfit, const float *__restrict__ tfit, float *__restrict__ Rcur,
    float *__restrict__ tcur, int *__restrict__ stopped, int *__restrict__ rounds,
    unsigned char *__restrict__ ok, int B) {
  const int b = blockIdx.x * GN_THREADS + threadIdx.x;
  if (b >= B || stopped[b] != 0) return;
  if (cnt[b] >= 3 && fit_ok[b] != 0) {
#pragma unroll
    for (int a = 0; a < 9; ++a) Rcur[b * 9 + a] = Rfit[b * 9 + a];
#pragma unroll
    for (int a = 0; a < 3; ++a) tcur[b * 3 + a] = tfit[b * 3 + a];
    rounds[b] += 1;
  } else {
    stopped[b] = 1;
    ok[b] = 0;
  }
}

// Launches 1-5 over `support`.  keys: B * T words; cells: 2 * B * T ints
// (counters, cursors); slot: B * M ints; sorted: B * M float4; bsum: B * nrun
// ints, nrun = ceil(T / block); state: nstate ints, status (B) first.  T is a
// power of two >= 2 M.
void launch_grid_nn_build(const float *support, const unsigned char *smask,
                          unsigned long long *keys, int *cells, int *slot, float *sorted,
                          int *bsum, int *state, long nstate, unsigned char *ok, float *Rcur,
                          float *tcur, const float *R0, const float *t0, int B, int M, int T,
                          float inv, hipStream_t stream) {
  const long BT = (long)B * T;
  int *cnt = cells, *cur = cells + BT;
  float4 *srt = reinterpret_cast<float4 *>(sorted);
  const int nblk = (M + GN_THREADS - 1) / GN_THREADS;
  const int nrun = (T + GN_THREADS - 1) / GN_THREADS;
  const dim3 block(GN_THREADS), pts(nblk, B), runs(nrun, B);
  long init_blocks = (BT + GN_THREADS - 1) / GN_THREADS;
  if (init_blocks > 8192) init_blocks = 8192;
  hipLaunchKernelGGL(gn_init_kernel, dim3((unsigned)init_blocks), block, 0, stream, keys, cnt, BT,
                     state, nstate, ok, Rcur, tcur, R0, t0, B);
  hipLaunchKernelGGL(gn_count_kernel, pts, block, 0, stream, support, smask, keys, cnt, slot,
                     state, ok, M, T, inv);
  hipLaunchKernelGGL(gn_scan_kernel, runs, block, 0, stream, cnt, cur, bsum, T);
  hipLaunchKernelGGL(gn_offset_kernel, dim3(B), dim3(GN_SCAN), 0, stream, bsum, nrun);
  hipLaunchKernelGGL(gn_scatter_kernel, pts, block, 0, stream, support, slot, cur, bsum, srt, M, T,
                     nrun);
}

// Launch 6.  mdst null: the plain search; otherwise the ICP flavour, which
// also fills mdst (B, Nq, 3), wgt (B, Nq) and adds to matched (B).
void launch_grid_nn_query(const float *query, const unsigned char *qmask, const float *R,
                          const float *t, const unsigned long long *keys, const int *cells,
                          const float *sorted, const int *bsum, const int *status,
                          unsigned char *ok, int *idx, float *d2, float *mdst, float *wgt,
                          int *matched, int B, int Nq, int M, int T, float inv, float r2, float th2,
                          hipStream_t stream) {
  const long BT = (long)B * T;
  const int *cnt = cells, *cur = cells + BT;
  const float4 *srt = reinterpret_cast<const float4 *>(sorted);
  const int nrun = (T + GN_THREADS - 1) / GN_THREADS;
  const dim3 block(GN_THREADS), qs((Nq + GN_THREADS - 1) / GN_THREADS, B);
  if (mdst == nullptr)
    hipLaunchKernelGGL(gn_query_kernel<false>, qs, block, 0, stream, query, qmask, R, t, srt, keys,
                       cnt, cur, bsum, status, ok, idx, d2, mdst, wgt, matched, Nq, M, T, nrun, inv,
                       r2, th2);
  else
    hipLaunchKernelGGL(gn_query_kernel<true>, qs, block, 0, stream, query, qmask, R, t, srt, keys,
                       cnt, cur, bsum, status, ok, idx, d2, mdst, wgt, matched, Nq, M, T, nrun, inv,
                       r2, th2);
}

void launch_icp_commit(const int *cnt, const unsigned char *fit_ok, const float *Rfit,
                       const float *tfit, float *Rcur, float *tcur, int *stopped, int *rounds,
                       unsigned char *ok, int B, hipStream_t stream) {
  hipLaunchKernelGGL(gn_commit_kernel, dim3((B + GN_THREADS - 1) / GN_THREADS), dim3(GN_THREADS),
                     0, stream, cnt, fit_ok, Rfit, tfit, Rcur, tcur, stopped, rounds, ok, B);
}
