// Shared tile core of the condenser kernels for gfx950: fused_condense and
// fused_embed_condense differ only in how a wave's A fragments arrive
// (streamed from the [M, K] concat tensor, or gathered from the embedding
// tables); the geometry, the glds weight stream, the MFMA chunk loop and
// the epilogue are the pieces below.
//
// Geometry per input width K (see fused_condense.hip for the reasoning):
//
//   layout                     K    NG   WS   waves  BM
//   max_passes=20              560  35   568  8      256
//   max_passes=20, ccs_bq      568  36   584  8      256
//   max_passes=32              872  55   888  4      128
//   max_passes=32, ccs_bq      880  55   888  4      128
//
// Every piece is __forceinline__ and takes wave-uniform values (tid, wave,
// m0, chunk) as plain ints; lane state comes from lane_recompute() at the
// point of use, so nothing lane-derived lives across the chunk loop.
//
// Only <hip/...> includes: the sanitizer harness includes the kernels from
// inside a namespace.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

using bf16 = __hip_bfloat16;

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int NC = 64;           // output-column chunk
constexpr int O_STRIDE = 72;     // output chunk image stride

template <int K>
struct CondCfg {
  static constexpr int NG = (K + 15) / 16;     // 16-elem K granules
  static constexpr int WS = 16 * NG + 8;       // weight image row stride
  static constexpr bool HALF = (K % 16) == 8;  // last granule half-filled
  static constexpr int NW = NG <= 36 ? 8 : 4;  // waves per block
  static constexpr int BM = 32 * NW;
  static constexpr int NT = 64 * NW;
  // Weight chunk = 64 rows x WS elems, copied in KiB units.
  static constexpr int UNITS = NC * WS * 2 / 1024;
  static_assert(K % 8 == 0, "rows must stay 16-B aligned");
  static_assert((NC * WS * 2) % 1024 == 0, "chunk must be whole KiB units");
  static_assert((NC * WS + BM * O_STRIDE) * 2 <= 160 * 1024, "LDS budget");
};

// Unhoistable lane id (volatile v_mbcnt): keeps lane-derived LDS addresses
// loop-local so nothing spills around the chunk loop (see fused_ffn_v3 —
// a spilled address's scratch reload carries a vmcnt(0) that drains the
// in-flight glds queue).
__device__ __forceinline__ int lane_recompute() {
  int l;
  asm volatile(
      "v_mbcnt_lo_u32_b32 %0, -1, 0\n\t"
      "v_mbcnt_hi_u32_b32 %0, -1, %0"
      : "=v"(l));
  return l;
}

// Weight chunk = 64 rows x WS elems = UNITS KiB-units; glds stream, each
// wave copying KiB-units wave, wave+NW, ... (per-lane 16-B granules).
template <int K>
__device__ __forceinline__ void cond_issue_w(
    const bf16* __restrict__ w, bf16 (&w_lds)[NC * CondCfg<K>::WS], int wave,
    int chunk) {
  using C = CondCfg<K>;
  constexpr int NW = C::NW;
  const int ln = lane_recompute();
  const bf16* src = w + (size_t)chunk * NC * C::WS;
  // Fully unrolled at 8 waves (9-10 trips). The 4-wave wide pair has 28
  // trips; unrolled whole, the 28 hoisted scalar base addresses overflow
  // the SGPR file, so it runs in groups of 4.
  constexpr int TRIPS = (C::UNITS + NW - 1) / NW;
  constexpr int UNROLL = NW == 8 ? TRIPS : 4;
#pragma unroll UNROLL
  for (int i = 0; i < TRIPS; ++i) {
    const int ck = wave + i * NW;
    if (ck < C::UNITS) {
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned*)(
              src + ck * 512 + ln * 8),
          (__attribute__((address_space(3))) unsigned*)(
              &w_lds[ck * 512]),
          16, 0, 0);
    }
  }
}

// Everything after the A fragments are in registers: the wait + barrier
// that ends the prologue (chunk 0 of the weight stream has landed), then
// per 64-column chunk the two-chain MFMA walk over both 32-column halves,
// the pos add + bf16 round into o_lds, the next chunk's glds issue, and
// the coalesced copy-out.
template <int K>
__device__ __forceinline__ void cond_chunk_loop(
    const bf16x8 (&af)[CondCfg<K>::NG], const bf16* __restrict__ w,
    const float* __restrict__ pos, bf16* __restrict__ out,
    bf16 (&w_lds)[NC * CondCfg<K>::WS],
    bf16 (&o_lds)[CondCfg<K>::BM * O_STRIDE], int M, int N, int Npad, int L,
    int tid, int wave, int m0) {
  using C = CondCfg<K>;
  constexpr int NG = C::NG;
  constexpr int W_STRIDE = C::WS;
  constexpr int BM = C::BM;
  constexpr int NT = C::NT;

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  const int nchunk = Npad / NC;
  for (int chunk = 0; chunk < nchunk; ++chunk) {
    const int ln = lane_recompute();
    const int c = ln & 31;
    const int hi = ln >> 5;
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {        // 32-col halves of the chunk
      const int colt = 32 * ch;
      const int ncol = chunk * NC + colt + c;
      f32x16 acc0 = {}, acc1 = {};
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int s = 0; s < NG; s += 2) {     // two independent chains
        const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(
            &w_lds[(colt + c) * W_STRIDE + 16 * s + 8 * hi]);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[s], b0, acc0,
                                                       0, 0, 0);
        if (s + 1 < NG) {
          const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(
              &w_lds[(colt + c) * W_STRIDE + 16 * (s + 1) + 8 * hi]);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[s + 1], b1,
                                                         acc1, 0, 0, 0);
        }
      }
      __builtin_amdgcn_s_setprio(0);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * hi + 32 * wave;
        float v = acc0[r] + acc1[r];
        if (pos != nullptr && ncol < N && m0 + row < M) {
          v += pos[(size_t)((m0 + row) % L) * N + ncol];
        }
        o_lds[row * O_STRIDE + colt + c] = __float2bfloat16(v);
      }
    }
    __syncthreads();  // o_lds complete; w_lds consumed
    if (chunk + 1 < nchunk) cond_issue_w<K>(w, w_lds, wave, chunk + 1);

    // Coalesced copy-out of this 64-col chunk, overlapping the glds fetch.
    const int n0 = chunk * NC;
    for (int idx = tid; idx < BM * (NC / 8); idx += NT) {
      const int row = idx / (NC / 8), c8 = idx % (NC / 8);
      if (m0 + row >= M) continue;
      const int col = n0 + 8 * c8;
      if (col >= N) continue;
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(
          &o_lds[row * O_STRIDE + 8 * c8]);
      if (col + 8 <= N) {
        *reinterpret_cast<bf16x8*>(
            out + (size_t)(m0 + row) * N + col) = v;
      } else {
        const unsigned short* vs =
            reinterpret_cast<const unsigned short*>(&v);
        for (int j = 0; j < 8 && col + j < N; ++j) {
          reinterpret_cast<unsigned short*>(
              out)[(size_t)(m0 + row) * N + col + j] = vs[j];
        }
      }
    }
    if (chunk + 1 < nchunk) {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
  }
}

}  // namespace
