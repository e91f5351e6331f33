// K7 backward (data gradient): one launch per 1x1-conv stack.
//
//   dpre[b, o, s] = dy[b, o, s] * (act == relu ? y[b, o, s] > 0 : 1)
//   dx_i[b, c, s] = sum_o W_i[o, c] * dpre[b, o, s]     per wanted part i
//
// replaces the composed backward of a pw_fwd stack (dy.contiguous, ATen
// threshold_backward, the point-major transpose, one hipBLASLt bmm per
// part -- each a launch-floor kernel at these sizes).
//
// Geometry follows pw_fwd.hip: 256 threads = 4 waves, one TC-column tile of
// one batch element per workgroup, the same TC policy.  The dpre tile is
// staged ONCE (masked on the way in; written back channel-major from the
// staged values when it differs from dy); the parts then run one after
// another over it, each staging its own (Co x Ci) weight.  Both operands
// lie in LDS as they lie in memory (pw_stage.h): k = o is the ROW index of
// the channel-major dpre tile and of the weight, so both fragments come
// from transposed LDS reads.  A point-major dy (B, S, Co) -- the SetConv
// fc1 case -- is already k-contiguous and is read by rows.
//
// MFMA operands: A = dpre (M = 16 columns s), B = W (N = 16 channels c),
// so each lane ends with FOUR CONSECUTIVE s of one channel: one packed
// 8-byte store per fragment.  bf16 operands, fp32 accumulate
// (v_mfma_f32_16x16x32_bf16), rounded once at the store.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <cstdlib>

#include "common.h"
#include "pw_stage.h"

typedef __attribute__((ext_vector_type(4))) float f32x4;

#define PB_THREADS PWS_THREADS
#define PB_MAXP 4

struct PwBwdPart {
  const void *w;  // (Co, Ci) bf16, rows ld elements apart
  void *dx;       // (B, Ci, S) bf16 contiguous
  int ci;
  int ld;
};

__device__ __forceinline__ unsigned pb_pack2(float lo, float hi) {
  return (unsigned)__bfloat16_as_ushort((__hip_bfloat16)lo) |
         ((unsigned)__bfloat16_as_ushort((__hip_bfloat16)hi) << 16);
}

// NCF: upper bound on 16-channel fragments of any part (wave-uniform
// guards skip the unused ones).
template <int NCF, int TC>
__global__ __launch_bounds__(PB_THREADS) void pw_bwd_kernel(
    PwBwdPart p0, PwBwdPart p1, PwBwdPart p2, PwBwdPart p3, int nparts,
    const __hip_bfloat16 *__restrict__ dy,  // (B, Co, S), or (B, S, Co) if pm
    const __hip_bfloat16 *__restrict__ y,   // same layout, or null (no ReLU)
    __hip_bfloat16 *__restrict__ dpre,      // channel-major rows, or null
    long dpre_bstride, int Co, long S, int pm, int w_off) {
  constexpr int COL16 = TC / 16;
  constexpr int CFG = 4 / COL16;  // wave groups along channel fragments
  constexpr int NCF_PER = (NCF + CFG - 1) / CFG;
  extern __shared__ __attribute__((aligned(16))) __hip_bfloat16 smem[];
  __hip_bfloat16 *s_d = smem;
  __hip_bfloat16 *s_w = smem + w_off;

  const int b = blockIdx.z;
  const long s0 = (long)blockIdx.x * TC;
  const int lane = lane_id();
  const int wv = wave_id();
  const int ct = wv % COL16;
  const int cf0 = (wv / COL16) * NCF_PER;
  const int cop = (Co + 31) & ~31;
  const int tcv = (S - s0) < TC ? (int)(S - s0) : TC;  // valid columns
  const int pitch_d = pm ? pws_row_pitch(cop) : pws_tr_pitch(TC);

  // ---- dpre tile, staged once
  if (pm) {
    const long go = ((long)b * S + s0) * Co;
    // only the mask load needs aligned rows
    const bool vec =
        y == nullptr || ((Co & 7) == 0 && ((size_t)y & 15) == 0);
    pws_stage_rows(s_d, pitch_d, dy + go, Co, tcv, TC, cop, Co, vec,
                   y != nullptr ? y + go : nullptr, nullptr, 0);
  } else {
    const long go = (long)b * Co * S + s0;
    __hip_bfloat16 *out =
        dpre != nullptr ? dpre + (long)b * dpre_bstride + s0 : nullptr;
    // the mask load and the dpre store want 16-byte-aligned rows; whole
    // chunks of a cut tile still go as vectors
    const bool vec =
        (y == nullptr && out == nullptr) ||
        ((S & 7) == 0 && (y == nullptr || ((size_t)y & 15) == 0) &&
         (out == nullptr ||
          (((size_t)dpre & 15) == 0 && (dpre_bstride & 7) == 0)));
    pws_stage_rows(s_d, pitch_d, dy + go, S, Co, cop, TC, tcv, vec,
                   y != nullptr ? y + go : nullptr, out, S);
  }
  __syncthreads();
  if (pm && dpre != nullptr) {
    // channel-major copy of the staged point-major tile: 8 columns of one
    // channel per thread, consecutive threads along s (coalesced rows)
    const bool vec =
        (S & 7) == 0 && ((size_t)dpre & 15) == 0 && (dpre_bstride & 7) == 0;
    __hip_bfloat16 *out = dpre + (long)b * dpre_bstride + s0;
    for (int i = threadIdx.x; i < Co * (TC / 8); i += PB_THREADS) {
      const int o = i / (TC / 8);
      const int c8 = (i % (TC / 8)) * 8;
      unsigned short e8[8];
#pragma unroll
      for (int e = 0; e < 8; ++e)
        e8[e] = ((const unsigned short *)s_d)[(long)(c8 + e) * pitch_d + o];
      if (vec && c8 + 8 <= tcv) {
        uint4 v;
        v.x = e8[0] | ((unsigned)e8[1] << 16);
        v.y = e8[2] | ((unsigned)e8[3] << 16);
        v.z = e8[4] | ((unsigned)e8[5] << 16);
        v.w = e8[6] | ((unsigned)e8[7] << 16);
        *(uint4 *)(out + (long)o * S + c8) = v;
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (c8 + e < tcv)
            ((unsigned short *)out)[(long)o * S + c8 + e] = e8[e];
      }
    }
  }

  // ---- parts
  const long sc = s0 + ct * 16 + (lane >> 4) * 4;  // first of this lane's 4 s
  const bool packed = (S & 3) == 0;
#pragma unroll
  for (int pi = 0; pi < PB_MAXP; ++pi) {
    if (pi >= nparts) break;
    // static selection (a runtime-indexed array would go to scratch)
    const PwBwdPart pp = pi == 0 ? p0 : pi == 1 ? p1 : pi == 2 ? p2 : p3;
    const int ci = pp.ci;
    const int ncf = (ci + 15) >> 4;
    const int pitch_w = pws_tr_pitch(ncf * 16);
    const __hip_bfloat16 *w = (const __hip_bfloat16 *)pp.w;
    if (pi > 0) __syncthreads();  // the previous part still reads s_w
    pws_stage_rows(s_w, pitch_w, w, pp.ld, Co, cop, ncf * 16, ci, true,
                   nullptr, nullptr, 0);
    __syncthreads();

    f32x4 acc[NCF_PER];
#pragma unroll
    for (int cf = 0; cf < NCF_PER; ++cf) acc[cf] = (f32x4)(0.f);
    for (int kb = 0; kb < cop; kb += 32) {
      const pws_bf16x8 afrag =
          pm ? pws_row_frag(s_d, pitch_d, ct * 16 + (lane & 15), kb, lane)
             : pws_tr_frag(s_d, pitch_d, kb, ct * 16, lane);
#pragma unroll
      for (int cf = 0; cf < NCF_PER; ++cf) {
        if (cf0 + cf < ncf) {  // wave-uniform
          const pws_bf16x8 bfrag =
              pws_tr_frag(s_w, pitch_w, kb, (cf0 + cf) * 16, lane);
          acc[cf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag, bfrag,
                                                            acc[cf], 0, 0, 0);
        }
      }
    }

    __hip_bfloat16 *dx = (__hip_bfloat16 *)pp.dx + (long)b * ci * S;
    // one uniform branch around the whole store loop, so the 8-byte store
    // is not folded into the per-element path
    if (packed) {
#pragma unroll
      for (int cf = 0; cf < NCF_PER; ++cf) {
        const int c = (cf0 + cf) * 16 + (lane & 15);
        if (cf0 + cf < ncf && c < ci && sc < S) {
          uint2 pk;
          pk.x = pb_pack2(acc[cf][0], acc[cf][1]);
          pk.y = pb_pack2(acc[cf][2], acc[cf][3]);
          *(uint2 *)&dx[(long)c * S + sc] = pk;
        }
      }
    } else {
#pragma unroll
      for (int cf = 0; cf < NCF_PER; ++cf) {
        const int c = (cf0 + cf) * 16 + (lane & 15);
        if (cf0 + cf < ncf && c < ci) {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (sc + e < S)
              dx[(long)c * S + sc + e] = (__hip_bfloat16)acc[cf][e];
        }
      }
    }
  }
}

// LDS halfwords of the dpre tile for a given tile width.
static inline long pb_tile_elems(int cop, int tc, int pm) {
  return pm ? (long)tc * pws_row_pitch(cop) : (long)cop * pws_tr_pitch(tc);
}

void launch_pw_bwd(const void **ws, void **dxs, const int *cis, const int *lds,
                   int nparts, const void *dy, const void *y, void *dpre,
                   long dpre_bstride, int B, int Co, long S, int point_major,
                   hipStream_t stream) {
  PwBwdPart p[PB_MAXP] = {};
  int ncf_max = 1;
  for (int i = 0; i < nparts; ++i) {
    p[i] = PwBwdPart{ws[i], dxs[i], cis[i], lds[i]};
    const int ncf = (cis[i] + 15) / 16;
    if (ncf > ncf_max) ncf_max = ncf;
  }
  const int cop = (Co + 31) & ~31;
  const long w_elems = nparts > 0 ? (long)cop * pws_tr_pitch(ncf_max * 16) : 0;
  // tile-width policy of pw_fwd.hip (PVRAFT_PW_TC=classic opts out there
  // and here)
  static const bool classic = [] {
    const char *e = getenv("PVRAFT_PW_TC");
    return e && e[0] == 'c';
  }();
  int tc = 64;
  if (!classic) {
    if ((long)B * ((S + 63) / 64) < 512) tc = 32;
    if ((long)B * ((S + 31) / 32) < 512) tc = 16;
  }
  // the widest weights (Co 256 x Ci 224) leave room for a narrow tile only
  const long lds_cap = 160 * 1024 - 1024;
  while (tc > 16 &&
         (pb_tile_elems(cop, tc, point_major) + w_elems) * 2 > lds_cap)
    tc >>= 1;
  // s_w starts on a 16-byte boundary: both tile sizes are multiples of 8
  const long w_off = pb_tile_elems(cop, tc, point_major);
  const size_t shmem = (size_t)(w_off + w_elems) * sizeof(__hip_bfloat16);
#define PB_LAUNCH_T(NCF, TC)                                                  \
  do {                                                                        \
    const dim3 grid((unsigned)((S + TC - 1) / TC), 1, B);                     \
    if (shmem > 64 * 1024) {                                                  \
      static bool raised = false;                                             \
      if (!raised) {                                                          \
        (void)hipFuncSetAttribute(                                            \
            reinterpret_cast<const void *>(&pw_bwd_kernel<NCF, TC>),          \
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_cap);        \
        raised = true;                                                        \
      }                                                                       \
    }                                                                         \
    hipLaunchKernelGGL((pw_bwd_kernel<NCF, TC>), grid, dim3(PB_THREADS),      \
                       shmem, stream, p[0], p[1], p[2], p[3], nparts,         \
                       (const __hip_bfloat16 *)dy, (const __hip_bfloat16 *)y, \
                       (__hip_bfloat16 *)dpre, dpre_bstride, Co, S,           \
                       point_major, (int)w_off);                              \
  } while (0)
#define PB_LAUNCH(NCF)                                                        \
  do {                                                                        \
    if (tc == 64) PB_LAUNCH_T(NCF, 64);                                       \
    else if (tc == 32) PB_LAUNCH_T(NCF, 32);                                  \
    else PB_LAUNCH_T(NCF, 16);                                                \
  } while (0)
  if (ncf_max <= 4) PB_LAUNCH(4);
  else if (ncf_max <= 8) PB_LAUNCH(8);
  else PB_LAUNCH(14);
#undef PB_LAUNCH
#undef PB_LAUNCH_T
}
