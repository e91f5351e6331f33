// K23: voxel-stratified sampling (absent in the reference): exactly m point
// indices per cloud, spatially even, deterministic, without a sort.
//
//   q = floor(fp32(x * inv)) per coordinate, inv = fp32(1) / fp32(voxel) from
//   the host.  Eligible: masked, finite, -2^20 <= q < 2^20 on all three axes.
//   Level-l cell of a point: int(q) >> l (arithmetic), l = 0 .. levels - 1.
//   tag_i = (mix(key(b) ^ i) << 32) | i, the 32-bit mixer of plane_fit.hip.
//   The representative of an occupied cell is its member with the smallest
//   tag; rank_i = number of levels at which i is a representative (the grids
//   are nested, so these are the levels 0 .. rank_i - 1); occupied[l] = number
//   of points with rank > l.  Selected: the first m' = min(m, eligible) points
//   in the order (rank descending, tag ascending), written in ascending index
//   order and padded with -1.
//   out: idx (B,m) int64, count (B) int32, rank (B,N) int32, occupied (B,L)
//
// 10 + levels launches.  Kernel boundaries and __syncthreads() inside one
// workgroup are the only synchronisation; no lane or workgroup ever waits for
// another one's progress.  All atomics are integer (compare-and-swap, min,
// add), so the result does not depend on the order in which they land.
//
//  1. vs_init_kernel     fills the three hash tables with the empty word and
//                        zeroes status, the eligible count, the radix
//                        histograms and occupied: every workspace word that is
//                        read later is written here or by a later kernel
//                        before its use.
//  2. vs_level0_kernel   one lane per point: eligibility, the 63-bit cell key
//                        (three 21-bit fields biased by 2^20), rank = 0 / -1,
//                        then the point finds or claims the slot of its key in
//                        table 0 and takes the minimum of its tag into it.
//                        A table has T >= 2 N slots (a power of two) per
//                        cloud; the slot comes from a 64-bit mix of the key
//                        (lattice inputs give arithmetic-progression keys).  A
//                        probe step is ONE compare-and-swap whose outcome is
//                        "claimed", "same key" or "other key: next slot"; it
//                        never retries a slot, and the loop is capped at T
//                        steps: a lane that hits the cap sets status[b].
//  3. vs_step_kernel     l = 1 .. levels, one launch each.  A point that
//                        entered level l - 1 is its representative iff the
//                        slot it remembered holds its own tag (final after the
//                        kernel boundary): rank = l, one add per wave (ballot
//                        count) to occupied[l - 1], and for l < levels it
//                        enters level l: (field >> l) keys, table l mod 3.
//                        Everyone else drops out.  The three tables rotate:
//                        level l - 1 is read, level l filled, and the slots of
//                        level l - 2 are reset, each by the one point that
//                        represented it (exactly the points that arrive here).
//                        The work shrinks with the occupied cells; a launch
//                        still covers all N lanes, the dead ones read one int.
//  4. vs_select_kernel   five launches: exact r-th smallest tag among the
//                        points of the cut rank c, most significant digit
//                        first, 12 bits a pass over the 60-bit (hash << 28 |
//                        index), same order as the tag because N < 2^27.
//                        Every workgroup first derives the digit of the pass
//                        before from that pass's finished histogram (4096
//                        bins, a block scan), so no launch sits between two
//                        passes; candidates are counted in an LDS histogram
//                        and flushed with one integer add per non-empty bin.
//                        c and r come from occupied and the eligible count: c
//                        is the largest rank with at least m' points at or
//                        above it, r = m' - (points above it).
//  5. vs_flag_kernel     selected = rank > c, or rank == c and tag <= the
//                        selected tag; flags and per-workgroup counts.
//  6. vs_scan_kernel     one wave per cloud: exclusive prefix of the
//                        workgroup counts, count[b] (-1 when status is set).
//  7. vs_write_kernel    idx in ascending order (workgroup offset + ballot
//                        prefix), -1 padding; with status set idx and rank
//                        are all -1.
//
// Measured (profiles/README.md: 0.096 ms a call at N = 8192, 0.263 ms at N =
// 131072, and a kernel trace).  Levels loop: one launch per level over all N
// lanes was kept.  The step launches are 58 - 69 % of the call, most of it in
// levels 1 - 5 where many points still insert; the last five levels, which a
// tail kernel (one workgroup per cloud looping over them) would replace, are
// 18 of 96 us and 30 of 263 us.  That kernel was not built: its own time is
// unknown, the numbers only bound its gain.  Select: every workgroup re-scans
// the 16 KB histogram of the pass before instead of a one-workgroup digit
// kernel between passes; passes with the scan take at most 0.6 us more than
// pass 0 without it, less than any launch in the trace.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), VGPRs /
// LDS bytes / scratch bytes: init 12 / 0 / 0, level0 16 / 0 / 0, step 20 / 0 / 0,
// select 30 / 16416 / 0, flag 29 / 32 / 0, scan 14 / 0 / 0, write 12 / 16 / 0;
// no AGPRs, 8 waves per SIMD everywhere.
#include <hip/hip_runtime.h>
#include "common.h"

#define VS_THREADS 256
#define VS_WAVES (VS_THREADS / WAVE)
#define VS_SCAN 64  // lanes of the workgroup-offset scan: one wave
#define VS_DIGIT 12
#define VS_BINS (1 << VS_DIGIT)
#define VS_PASSES 5  // 5 x 12 bits = the 60-bit order word
#define VS_PER_LANE (VS_BINS / VS_THREADS)
#define VS_RANGE (1 << 20)
#define VS_FIELD 0x1fffffull
#define VS_EMPTY (~0ull)  // no key (bit 63 clear) and no tag (index < 2^27) equals it
// per-cloud ints: status, eligible, (prefix lo, prefix hi, r, c) entering
// pass 0 .. VS_PASSES, then VS_PASSES histograms
#define VS_META_STATE 2
#define VS_META_HIST (VS_META_STATE + 4 * (VS_PASSES + 1))
#define VS_META (VS_META_HIST + VS_PASSES * VS_BINS)

typedef unsigned long long vs_u64;

int voxel_sample_block() { return VS_THREADS; }
int voxel_sample_scan() { return VS_SCAN; }
long voxel_sample_meta() { return VS_META; }

DEV_INLINE unsigned vs_mix(unsigned x) {
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

DEV_INLINE unsigned vs_cloud_key(unsigned seed, int b) {
  return vs_mix(seed ^ vs_mix((unsigned)b * 0x9E3779B1u + 1u));
}

// slot hash: the 64-bit finaliser of the same family
DEV_INLINE unsigned vs_slot_hash(vs_u64 k) {
  k ^= k >> 33;
  k *= 0xFF51AFD7ED558CCDull;
  k ^= k >> 33;
  k *= 0xC4CEB9FE1A85EC53ull;
  k ^= k >> 33;
  return (unsigned)k;
}

DEV_INLINE vs_u64 vs_level_key(vs_u64 key0, int l) {
  const vs_u64 fx = key0 >> 42, fy = (key0 >> 21) & VS_FIELD, fz = key0 & VS_FIELD;
  return ((fx >> l) << 42) | ((fy >> l) << 21) | (fz >> l);
}

// Finds or claims the slot of `key`, takes min(tag) into it; -1 at the cap.
DEV_INLINE int vs_insert(vs_u64 *keys, vs_u64 *tags, int T, vs_u64 key, vs_u64 tag) {
  unsigned s = vs_slot_hash(key) & (unsigned)(T - 1);
  for (int step = 0; step < T; ++step) {
    vs_u64 seen = VS_EMPTY;
    const bool claimed = __hip_atomic_compare_exchange_strong(
        keys + s, &seen, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (claimed || seen == key) {
      __hip_atomic_fetch_min(tags + s, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return (int)s;
    }
    s = (s + 1u) & (unsigned)(T - 1);
  }
  return -1;
}

__global__ __launch_bounds__(VS_THREADS) void vs_init_kernel(
    vs_u64 *__restrict__ tab, long tab_pairs, int *__restrict__ meta, long meta_words,
    int *__restrict__ occ, long occ_words) {
  const long t = (long)blockIdx.x * VS_THREADS + threadIdx.x;
  const long stride = (long)gridDim.x * VS_THREADS;
  ulonglong2 *t2 = reinterpret_cast<ulonglong2 *>(tab);
  for (long j = t; j < tab_pairs; j += stride) t2[j] = make_ulonglong2(VS_EMPTY, VS_EMPTY);
  for (long j = t; j < meta_words; j += stride) meta[j] = 0;
  for (long j = t; j < occ_words; j += stride) occ[j] = 0;
}

__global__ __launch_bounds__(VS_THREADS) void vs_level0_kernel(
    const float *__restrict__ xyz,           // (B, N, 3)
    const unsigned char *__restrict__ mask,  // (B, N) or null
    vs_u64 *keys, vs_u64 *tags,              // table 0: (B, T) each
    vs_u64 *__restrict__ key0,               // (B, N)
    int *__restrict__ cur,                   // (B, N)
    int *__restrict__ rank,                  // (B, N)
    int *meta, int N, int T, float inv, unsigned seed) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * VS_THREADS + threadIdx.x;
  int *mb = meta + (long)b * VS_META;
  bool el = false;
  if (i < N) {
    const long g = (long)b * N + i;
    const float x = xyz[g * 3 + 0], y = xyz[g * 3 + 1], z = xyz[g * 3 + 2];
    const float qx = floorf(x * inv), qy = floorf(y * inv), qz = floorf(z * inv);
    const float lo = -(float)VS_RANGE, hi = (float)VS_RANGE;
    el = (mask == nullptr || mask[g] != 0) && isfinite(x) && isfinite(y) && isfinite(z) &&
         qx >= lo && qx < hi && qy >= lo && qy < hi && qz >= lo && qz < hi;
    vs_u64 key = 0;
    int slot = -1;
    if (el) {
      key = ((vs_u64)((int)qx + VS_RANGE) << 42) | ((vs_u64)((int)qy + VS_RANGE) << 21) |
            (vs_u64)((int)qz + VS_RANGE);
      const vs_u64 tag = ((vs_u64)vs_mix(vs_cloud_key(seed, b) ^ (unsigned)i) << 32) | (unsigned)i;
      slot = vs_insert(keys + (long)b * T, tags + (long)b * T, T, key, tag);
      if (slot < 0) __hip_atomic_store(mb + 0, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    key0[g] = key;
    cur[g] = slot;
    rank[g] = el ? 0 : -1;
  }
  const unsigned long long bal = __ballot(el);
  if (lane_id() == 0 && bal != 0) atomicAdd(mb + 1, __popcll(bal));
}

__global__ __launch_bounds__(VS_THREADS) void vs_step_kernel(
    const vs_u64 *__restrict__ key0,
    const vs_u64 *__restrict__ tags_prev,  // level l - 1: read
    vs_u64 *keys_new, vs_u64 *tags_new,    // level l: filled
    vs_u64 *__restrict__ keys_old, vs_u64 *__restrict__ tags_old,  // level l - 2: reset
    int *__restrict__ cur, int *__restrict__ prev, int *__restrict__ rank,
    int *__restrict__ occ, int *meta, int N, int T, int l, int L, unsigned seed) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * VS_THREADS + threadIdx.x;
  bool rep = false;
  if (i < N) {
    const long g = (long)b * N + i;
    const long tb = (long)b * T;
    const int s1 = cur[g];
    if (s1 >= 0) {
      if (l >= 2) {
        const int s2 = prev[g];
        keys_old[tb + s2] = VS_EMPTY;
        tags_old[tb + s2] = VS_EMPTY;
      }
      const vs_u64 tag = ((vs_u64)vs_mix(vs_cloud_key(seed, b) ^ (unsigned)i) << 32) | (unsigned)i;
      rep = tags_prev[tb + s1] == tag;
      int s0 = -1;
      if (rep) {
        rank[g] = l;
        if (l < L) {
          s0 = vs_insert(keys_new + tb, tags_new + tb, T, vs_level_key(key0[g], l), tag);
          if (s0 < 0)
            __hip_atomic_store(meta + (long)b * VS_META, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      prev[g] = s1;
      cur[g] = s0;
    }
  }
  const unsigned long long bal = __ballot(rep);
  if (lane_id() == 0 && bal != 0) atomicAdd(occ + (long)b * L + (l - 1), __popcll(bal));
}

// Exclusive prefix of v over the workgroup's VS_THREADS lanes.
DEV_INLINE int vs_block_excl(int v, int *wsum) {
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
  for (int w = 0; w < VS_WAVES; ++w) base += w < wave_id() ? wsum[w] : 0;
  __syncthreads();  // wsum may be reused
  return base + x - v;
}

// The state entering pass p, in st[0..3] = (prefix lo, prefix hi, r, c), the
// same in every workgroup of the launch: for p = 0 the cut from occupied and
// the eligible count, else the state of pass p - 1 advanced by the digit that
// its finished histogram selects.  Workgroup 0 records it for the next launch.
DEV_INLINE void vs_enter_pass(int *mb, const int *occ_b, int L, long m, int p, int *st, int *wsum) {
  const int tid = threadIdx.x;
  if (p == 0) {
    if (tid == 0) {
      const int elig = mb[1];
      const int mp = m < (long)elig ? (int)m : elig;
      int c = 0;  // largest rank with at least m' points at or above it
      for (int r = 1; r <= L; ++r)
        if (occ_b[r - 1] >= mp) c = r;
      const int above = c < L ? occ_b[c] : 0;
      st[0] = 0;
      st[1] = 0;
      st[2] = mp - above;
      st[3] = c;
    }
    __syncthreads();
  } else {
    const int *sp = mb + VS_META_STATE + 4 * (p - 1);
    const vs_u64 prefix = ((vs_u64)(unsigned)sp[1] << 32) | (unsigned)sp[0];
    const int r = sp[2];
    if (tid == 0) {
      const vs_u64 np = prefix << VS_DIGIT;  // r == 0 (nothing eligible): digit 0
      st[0] = (int)(unsigned)np;
      st[1] = (int)(unsigned)(np >> 32);
      st[2] = 0;
      st[3] = sp[3];
    }
    const int *h = mb + VS_META_HIST + (p - 1) * VS_BINS + tid * VS_PER_LANE;
    int hv[VS_PER_LANE];
    int t = 0;
#pragma unroll
    for (int k = 0; k < VS_PER_LANE; ++k) {
      hv[k] = h[k];
      t += hv[k];
    }
    const int ex = vs_block_excl(t, wsum);  // its barriers order the defaults above
    if (r >= 1 && ex < r && r <= ex + t) {  // exactly one lane
      int cum = ex, d = 0, nr = 0;
      bool found = false;
#pragma unroll
      for (int k = 0; k < VS_PER_LANE; ++k) {
        if (!found && cum + hv[k] >= r) {
          found = true;
          d = tid * VS_PER_LANE + k;
          nr = r - cum;
        }
        cum += hv[k];
      }
      const vs_u64 np = (prefix << VS_DIGIT) | (vs_u64)d;
      st[0] = (int)(unsigned)np;
      st[1] = (int)(unsigned)(np >> 32);
      st[2] = nr;
    }
    __syncthreads();
  }
  if (blockIdx.x == 0 && tid < 4) mb[VS_META_STATE + 4 * p + tid] = st[tid];
}

DEV_INLINE vs_u64 vs_order_word(unsigned seed, int b, int i) {
  return ((vs_u64)vs_mix(vs_cloud_key(seed, b) ^ (unsigned)i) << 28) | (unsigned)i;
}

__global__ __launch_bounds__(VS_THREADS) void vs_select_kernel(
    const int *__restrict__ rank, const int *__restrict__ occ, int *meta, int N, int L,
    long m, int p, unsigned seed) {
  __shared__ int hist[VS_BINS];
  __shared__ int wsum[VS_WAVES];
  __shared__ int st[4];
  const int b = blockIdx.y;
  const int tid = threadIdx.x;
  const int i = blockIdx.x * VS_THREADS + tid;
  int *mb = meta + (long)b * VS_META;
#pragma unroll
  for (int k = 0; k < VS_PER_LANE; ++k) hist[tid * VS_PER_LANE + k] = 0;
  vs_enter_pass(mb, occ + (long)b * L, L, m, p, st, wsum);  // ends after a barrier
  const vs_u64 prefix = ((vs_u64)(unsigned)st[1] << 32) | (unsigned)st[0];
  const int c = st[3];
  if (i < N && rank[(long)b * N + i] == c) {
    const vs_u64 w = vs_order_word(seed, b, i);
    const int top = VS_DIGIT * (VS_PASSES - p);  // bits below the prefix
    if (p == 0 || (w >> top) == prefix)
      atomicAdd(&hist[(int)((w >> (top - VS_DIGIT)) & (VS_BINS - 1))], 1);
  }
  __syncthreads();
  int *gh = mb + VS_META_HIST + p * VS_BINS;
#pragma unroll
  for (int k = 0; k < VS_PER_LANE; ++k) {
    const int v = hist[tid * VS_PER_LANE + k];
    if (v != 0) atomicAdd(gh + tid * VS_PER_LANE + k, v);
  }
}

__global__ __launch_bounds__(VS_THREADS) void vs_flag_kernel(
    const int *__restrict__ rank, const int *__restrict__ occ, int *meta,
    unsigned char *__restrict__ sel, int *__restrict__ bsum, int N, int L, long m,
    unsigned seed) {
  __shared__ int wsum[VS_WAVES];
  __shared__ int st[4];
  const int b = blockIdx.y;
  const int tid = threadIdx.x;
  const int i = blockIdx.x * VS_THREADS + tid;
  int *mb = meta + (long)b * VS_META;
  vs_enter_pass(mb, occ + (long)b * L, L, m, VS_PASSES, st, wsum);
  const vs_u64 cutw = ((vs_u64)(unsigned)st[1] << 32) | (unsigned)st[0];
  const int c = st[3];
  const bool failed = mb[0] != 0;  // final: every insert ran in an earlier launch
  bool s = false;
  if (i < N) {
    const int r = rank[(long)b * N + i];
    s = !failed && r >= 0 && (r > c || (r == c && vs_order_word(seed, b, i) <= cutw));
    sel[(long)b * N + i] = s ? 1 : 0;
  }
  const unsigned long long bal = __ballot(s);
  if (lane_id() == 0) wsum[wave_id()] = __popcll(bal);
  __syncthreads();
  if (tid == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < VS_WAVES; ++w) t += wsum[w];
    bsum[(long)b * gridDim.x + blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(VS_SCAN) void vs_scan_kernel(
    int *__restrict__ bsum, const int *__restrict__ meta, int *__restrict__ count, int nblk) {
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  bsum += (long)b * nblk;
  int run = 0;
  for (int base = 0; base < nblk; base += VS_SCAN) {
    const int j = base + lane;
    const int v = j < nblk ? bsum[j] : 0;
    int x = v;
#pragma unroll
    for (int off = 1; off < VS_SCAN; off <<= 1) {
      const int y = __shfl_up(x, off, WAVE);
      if (lane >= off) x += y;
    }
    if (j < nblk) bsum[j] = run + x - v;
    run += __shfl(x, VS_SCAN - 1, WAVE);
  }
  if (lane == 0) count[b] = meta[(long)b * VS_META] != 0 ? -1 : run;
}

__global__ __launch_bounds__(VS_THREADS) void vs_write_kernel(
    const unsigned char *__restrict__ sel, const int *__restrict__ bsum,
    const int *__restrict__ count, long *__restrict__ idx, int *__restrict__ rank, int N,
    long m) {
  __shared__ int wsum[VS_WAVES];
  const int b = blockIdx.y;
  const int tid = threadIdx.x;
  const int i = blockIdx.x * VS_THREADS + tid;
  const int cnt = count[b];
  const bool s = i < N && sel[(long)b * N + i] != 0;
  const unsigned long long bal = __ballot(s);
  if (lane_id() == 0) wsum[wave_id()] = __popcll(bal);
  __syncthreads();
  long pos = bsum[(long)b * gridDim.x + blockIdx.x];
#pragma unroll
  for (int w = 0; w < VS_WAVES; ++w) pos += w < wave_id() ? wsum[w] : 0;
  pos += __popcll(bal & ((1ull << lane_id()) - 1ull));
  idx += (long)b * m;
  if (s && pos < m) idx[pos] = i;
  if (cnt < 0 && i < N) rank[(long)b * N + i] = -1;
  const long filled = cnt < 0 ? 0 : cnt;
  for (long j = filled + (long)blockIdx.x * VS_THREADS + tid; j < m; j += (long)gridDim.x * VS_THREADS)
    idx[j] = -1;
}

// tab: 6 * B * T words (keys of tables 0..2, then their tags); key0: B * N
// words; slots: 2 * B * N ints (cur, prev); sel: B * N bytes; bsum: B * nblk
// ints; meta: B * voxel_sample_meta() ints.  T is a power of two >= 2 N.
void launch_voxel_sample(const float *xyz, const unsigned char *mask, unsigned long long *tab,
                         unsigned long long *key0, int *slots, unsigned char *sel, int *bsum,
                         int *meta, long *idx, int *count, int *rank, int *occ, int B, int N,
                         int T, long m, int L, float inv, unsigned seed, hipStream_t stream) {
  const long BT = (long)B * T, BN = (long)B * N;
  vs_u64 *keys[3] = {tab, tab + BT, tab + 2 * BT};
  vs_u64 *tags[3] = {tab + 3 * BT, tab + 4 * BT, tab + 5 * BT};
  int *cur = slots, *prev = slots + BN;
  const int nblk = (N + VS_THREADS - 1) / VS_THREADS;
  const dim3 block(VS_THREADS), pts(nblk, B);
  const long tab_pairs = 3 * BT;  // 6 BT words, T is even
  long init_blocks = (tab_pairs + VS_THREADS - 1) / VS_THREADS;
  if (init_blocks > 8192) init_blocks = 8192;
  hipLaunchKernelGGL(vs_init_kernel, dim3((unsigned)init_blocks), block, 0, stream, tab, tab_pairs,
                     meta, (long)B * VS_META, occ, (long)B * L);
  hipLaunchKernelGGL(vs_level0_kernel, pts, block, 0, stream, xyz, mask, keys[0], tags[0], key0,
                     cur, rank, meta, N, T, inv, seed);
  for (int l = 1; l <= L; ++l)
    hipLaunchKernelGGL(vs_step_kernel, pts, block, 0, stream, key0, tags[(l - 1) % 3], keys[l % 3],
                       tags[l % 3], keys[(l + 1) % 3], tags[(l + 1) % 3], cur, prev, rank, occ,
                       meta, N, T, l, L, seed);
  for (int p = 0; p < VS_PASSES; ++p)
    hipLaunchKernelGGL(vs_select_kernel, pts, block, 0, stream, rank, occ, meta, N, L, m, p, seed);
  hipLaunchKernelGGL(vs_flag_kernel, pts, block, 0, stream, rank, occ, meta, sel, bsum, N, L, m,
                     seed);
  hipLaunchKernelGGL(vs_scan_kernel, dim3(B), dim3(VS_SCAN), 0, stream, bsum, meta, count, nblk);
  hipLaunchKernelGGL(vs_write_kernel, pts, block, 0, stream, sel, bsum, count, idx, rank, N, m);
}
