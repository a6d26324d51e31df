// Fused FFN v3 for gfx950: 256-row tiles, register-resident h, glds weights.
//
// One-shot sequencing of the tile core in ffn_tile.h (design, layout and
// LDS budget are described there): one block per 256-row tile stages x
// through LDS, walks the 32 hidden chunks with double-buffered weight DMA
// and stores with the 2-byte epilogue. Fallback for fused_ffn_v5 and its
// bitwise oracle.

#ifndef DC_SAN_MAIN
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#endif
#include <hip/hip_runtime.h>
#include "ffn_tile.h"

namespace {

__global__ __launch_bounds__(512, 1) void fused_ffn_v3_kernel(
    const bf16* __restrict__ x, const bf16* __restrict__ w1,
    const bf16* __restrict__ w2, const float* __restrict__ b2,
    bf16* __restrict__ out, int M, float alpha) {
  __shared__ __attribute__((aligned(16))) bf16 smem[LDS_ELEMS];

  // wave id lives in an SGPR (readfirstlane) — free to keep live.
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m0 = blockIdx.x * BM;

  bf16x8 af[18];
  stage_x_issue_chunk0(smem, x, w1, w2, m0, M, wave, af);

  f32x16 oacc[9] = {};

  for (int chunk = 0; chunk < NCHUNK; ++chunk) {
    const int ln = lane_recompute();
    const int c = ln & 31;   // loop-local, dead at the backedge ->
    const int hi = ln >> 5;  // nothing to spill
    const int buf = chunk & 1;
    const bool more = chunk + 1 < NCHUNK;
    if (more) {
      issue_w1(smem, w1, wave, chunk + 1, buf ^ 1);
      issue_w2(smem, w2, wave, chunk + 1, buf ^ 1);
    }
    const bf16* w1buf = &smem[OFF_W1 + buf * W1_ELEMS];
    const bf16* w2buf = &smem[OFF_W2 + buf * W2_ELEMS];

    // Per 32-hidden tile: B1, ReLU, repack, then its two B2 k-steps —
    // only one tile's st/pa live at a time.
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const f32x16 acc = b1_step(w1buf, af, t, c, hi);
      f32x16 st;
#pragma unroll
      for (int r = 0; r < 16; ++r) st[r] = acc[r] > 0.f ? acc[r] : 0.f;
      bf16x8 pa[2];
      t12_repack(st, pa);
      b2_step(w2buf, pa, oacc, t, c, hi);
    }

    // Next chunk's 11 DMA groups must have landed; raw barrier (a
    // __syncthreads would also drain nothing extra here — vmcnt(0) is
    // already required since both buffers' DMAs are the only vmem).
    if (more) {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
  }

  // Epilogue: b2 + ReZero alpha + residual.
  store_tile_2b(out, oacc, m0, M, wave,
                [&](int col, size_t off, float acc) {
                  return __bfloat162float(x[off]) + alpha * (acc + b2[col]);
                });
}

}  // namespace

#ifndef DC_SAN_MAIN

at::Tensor fused_ffn_v3(at::Tensor x, at::Tensor w1, at::Tensor w2,
                        at::Tensor b2, double alpha) {
  TORCH_CHECK(x.is_cuda() && x.dtype() == at::kBFloat16,
              "x must be bf16 on device");
  auto xc = x.contiguous();
  const int K = xc.size(-1);
  const int M = xc.numel() / K;
  TORCH_CHECK(K == K1, "fused_ffn_v3 requires width 280");
  TORCH_CHECK(w1.size(0) == NHID && w1.size(1) == K1P,
              "w1 must be [2048, 296] with b1 folded into column 287");
  TORCH_CHECK(w2.size(0) == 320 && w2.size(1) == NHID,
              "w2 must be padded [320, 2048]");
  TORCH_CHECK(b2.numel() >= NOUT, "b2 must cover 280 outputs");
  auto b2c = b2.contiguous();
  TORCH_CHECK(b2c.dtype() == at::kFloat, "b2 must be fp32");
  auto out = at::empty_like(xc);
  dim3 grid((M + BM - 1) / BM);
  dim3 block(512);
  hipStream_t stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(fused_ffn_v3_kernel, grid, block, 0, stream,
                     reinterpret_cast<bf16*>(xc.data_ptr()),
                     reinterpret_cast<bf16*>(w1.data_ptr()),
                     reinterpret_cast<bf16*>(w2.data_ptr()),
                     b2c.data_ptr<float>(),
                     reinterpret_cast<bf16*>(out.data_ptr()), M,
                     (float)alpha);
  return out;
}

#endif  // DC_SAN_MAIN
