// Fused condenser GEMM for gfx950: out = x @ W^T + pos  (K3 + K4).
//
// The production model's no-bias condenser Linear (networks.py:426-434,
// 509-516: [B*L, K] x [K, 280]) plus the sinusoidal position-encoding
// add (networks.py:203-205) fused into the epilogue — the last library
// kernel (hipBLASLt) and the last standalone elementwise op on the serving
// path, replaced by one MFMA kernel reusing the fused_linear structure.
//
// The kernel is a template on the concat width K, instantiated for the
// four input layouts the project serves:
//
//   layout                     K    NG   WS   waves  BM
//   max_passes=20              560  35   568  8      256
//   max_passes=20, ccs_bq      568  36   584  8      256
//   max_passes=32              872  55   888  4      128
//   max_passes=32, ccs_bq      880  55   888  4      128
//
// NG = ceil(K/16) 16-element K granules; WS = 16*NG + 8 is the weight
// image row stride (global and LDS).
//
// Shape specifics vs fused_linear (K = 280 there):
//  * Each wave OWNS one 32-row group and walks both 32-column halves of
//    the 64-col weight chunk. With 8 waves (BM = 256) that halves weight
//    refetch vs BM=128: 2.3 GB/call at M = 1.6 M rows.
//  * A-fragments: NG bf16x8 granules per lane, register-resident across
//    all N chunks (x is read from HBM exactly once). At NG = 35/36 that is
//    140/144 VGPRs: 8 waves, 2 per SIMD, 256 registers each. At NG = 55 it
//    is 220 VGPRs, which does not fit a 256-register wave next to the two
//    accumulators, so the wide pair runs 4 waves per block (one per SIMD,
//    the full 512-entry file, accumulators free to live in AGPRs).
//  * One block per CU either way (LDS: 64 x WS weight image + BM x 72 out
//    image = 109.6 / 111.6 / 132.1 KB).
//  * The NG-step dependent MFMA chain is split into two independent
//    accumulators (even/odd granules) merged at the epilogue, since at
//    <= 2 waves/SIMD there is less latency cover than fused_linear's 4.
//  * Epilogue adds pos[(m0+row) % L, col] (fp32 table) before the bf16
//    round — the separate "+ pos" elementwise kernel disappears.
//
// Half granule: for K = 8 mod 16 (568, 872) elements K .. K+7 of the last
// granule lie outside the row. Lanes with hi = 1 hold exactly that half;
// their last A fragment is zeroed in registers and the load is NOT issued
// (the over-read would return the next row's data — 0 x NaN is NaN — and
// leaves the tensor on the last row). The B side still reads
// w_lds[.. + 16*(NG-1) + 8], which WS >= 16*NG keeps inside the row's own
// (host-zeroed) image.
//
// W arrives host-padded to [Npad, WS] (Npad mult of 64) with row n =
// condenser.weight[n, :K], zero elsewhere — see runner.build_condense_image.

#ifndef DC_SAN_MAIN
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#endif
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include "condense_tile.h"

namespace {

template <int K>
__global__ __launch_bounds__(CondCfg<K>::NT, 1) void fused_condense_kernel(
    const bf16* __restrict__ x, const bf16* __restrict__ w,
    const float* __restrict__ pos, bf16* __restrict__ out,
    int M, int N, int Npad, int L) {
  using C = CondCfg<K>;
  constexpr int NG = C::NG;
  constexpr int W_STRIDE = C::WS;
  constexpr int BM = C::BM;
  __shared__ __attribute__((aligned(16))) bf16 w_lds[NC * W_STRIDE];
  __shared__ __attribute__((aligned(16))) bf16 o_lds[BM * O_STRIDE];

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0 = blockIdx.x * BM;

  cond_issue_w<K>(w, w_lds, wave, 0);

  // A-fragments straight from global: lane (c, hi) of wave w owns row
  // m0 + 32w + c, granules 16s + 8hi — the wave collectively reads its
  // contiguous 32-row x 2K-B region, so every DRAM sector is consumed
  // exactly once; no LDS bounce, no staging barriers (the 4-pass
  // stage-through-w_lds prologue this replaces cost ~1/3 of the kernel).
  bf16x8 af[NG];
  {
    const int ln = lane_recompute();
    const int row = m0 + 32 * wave + (ln & 31);
    constexpr int NFULL = C::HALF ? NG - 1 : NG;
    if (row < M) {
      const bf16* xr = x + (size_t)row * K + 8 * (ln >> 5);
#pragma unroll
      for (int s = 0; s < NFULL; ++s) {
        af[s] = *reinterpret_cast<const bf16x8*>(xr + 16 * s);
      }
    } else {
#pragma unroll
      for (int s = 0; s < NFULL; ++s) af[s] = bf16x8{};
    }
    if constexpr (C::HALF) {
      // Elements K-8 .. K-1 belong to the hi = 0 lanes; the hi = 1 half
      // (K .. K+7) is past the row end: zero, and no load.
      af[NG - 1] = bf16x8{};
      if (row < M && (ln >> 5) == 0) {
        af[NG - 1] = *reinterpret_cast<const bf16x8*>(
            x + (size_t)row * K + 16 * (NG - 1));
      }
    }
  }
  cond_chunk_loop<K>(af, w, pos, out, w_lds, o_lds, M, N, Npad, L, tid, wave,
                     m0);
}

// Explicit instantiations: exactly the four served widths.
#define DC_CONDENSE_INST(K)                                       \
  template __global__ void fused_condense_kernel<K>(              \
      const bf16* __restrict__, const bf16* __restrict__,         \
      const float* __restrict__, bf16* __restrict__, int, int, int, int)
DC_CONDENSE_INST(560);
DC_CONDENSE_INST(568);
DC_CONDENSE_INST(872);
DC_CONDENSE_INST(880);
#undef DC_CONDENSE_INST

}  // namespace

#ifndef DC_SAN_MAIN

namespace {

template <int K>
void launch_condense(const at::Tensor& xc, const at::Tensor& w,
                     const float* pos_ptr, at::Tensor& out, int M, int N,
                     int Npad, int L) {
  using C = CondCfg<K>;
  TORCH_CHECK(w.size(1) == C::WS, "fused_condense: width-", K,
              " input needs a weight image of row stride ", C::WS,
              ", got ", w.size(1));
  dim3 grid((M + C::BM - 1) / C::BM);
  dim3 block(C::NT);
  hipStream_t stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(fused_condense_kernel<K>, grid, block, 0, stream,
                     reinterpret_cast<bf16*>(xc.data_ptr()),
                     reinterpret_cast<bf16*>(w.data_ptr()), pos_ptr,
                     reinterpret_cast<bf16*>(out.data_ptr()), M, N, Npad,
                     L > 0 ? L : 1);
}

}  // namespace

at::Tensor fused_condense(at::Tensor x, at::Tensor w, at::Tensor pos,
                          int64_t n_out, int64_t seq_len) {
  TORCH_CHECK(x.is_cuda() && x.dtype() == at::kBFloat16,
              "x must be bf16 on device");
  auto xc = x.contiguous();
  const int K = xc.size(-1);
  TORCH_CHECK(K == 560 || K == 568 || K == 872 || K == 880,
              "fused_condense requires input width 560, 568, 872 or 880, "
              "got ", K);
  const int M = xc.numel() / K;
  TORCH_CHECK(w.is_cuda() && w.dim() == 2 && w.is_contiguous() &&
                  w.dtype() == at::kBFloat16 && w.size(0) % NC == 0,
              "w must be contiguous bf16 [Npad (mult of 64), WS] on device");
  const int Npad = w.size(0);
  const int N = (int)n_out;
  TORCH_CHECK(N <= Npad, "n_out exceeds padded weight rows");
  const int L = (int)seq_len;
  const float* pos_ptr = nullptr;
  at::Tensor pc;
  if (pos.defined() && pos.numel() > 0) {
    pc = pos.contiguous();
    TORCH_CHECK(pc.dtype() == at::kFloat && pc.size(-1) == N &&
                    pc.numel() >= (int64_t)L * N && L > 0,
                "pos must be fp32 [>=L, N]");
    pos_ptr = pc.data_ptr<float>();
  }
  auto out = at::empty({M, N}, xc.options());
  if (M == 0) return out;
  switch (K) {
    case 560: launch_condense<560>(xc, w, pos_ptr, out, M, N, Npad, L); break;
    case 568: launch_condense<568>(xc, w, pos_ptr, out, M, N, Npad, L); break;
    case 872: launch_condense<872>(xc, w, pos_ptr, out, M, N, Npad, L); break;
    default:  launch_condense<880>(xc, w, pos_ptr, out, M, N, Npad, L); break;
  }
  return out;
}

#endif  // DC_SAN_MAIN
