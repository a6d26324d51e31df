// ABLATION build of fused_ffn_v3 (perf diagnosis only, not shipped in
// the serving path): template<int MODE> — 0 full (= v3, bitwise), 1 B1-only
// (B2 MFMAs skipped, pa kept live via asm), 2 B2-only (pa fed from a zero
// acc, B1 skipped), 3 loads/loops/barriers only, 4 loads + VALU spin,
// 6 per-block chunk rotation. Guide rule 17: skipped values are kept live
// with empty asm so upstream work is not DCEd. Everything but the MODE
// switches comes from ffn_tile.h.

#ifndef DC_SAN_MAIN
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#endif
#include <hip/hip_runtime.h>
#include "ffn_tile.h"

namespace {

template <int MODE>
__global__ __launch_bounds__(512, 1) void ffn_ablate_kernel(
    const bf16* __restrict__ x, const bf16* __restrict__ w1,
    const bf16* __restrict__ w2, const float* __restrict__ b2,
    bf16* __restrict__ out, int M, float alpha) {
  __shared__ __attribute__((aligned(16))) bf16 smem[LDS_ELEMS];

  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m0 = blockIdx.x * BM;

  bf16x8 af[18];
  stage_x_issue_chunk0(smem, x, w1, w2, m0, M, wave, af);

  f32x16 oacc[9] = {};

  // MODE 6: rotate the chunk order per block so the XCD-level weight
  // working set is the whole 2.5 MB steadily (L2-resident) instead of
  // a synchronized-then-strangled walk.
  const int rot = (MODE == 6) ? (int)(blockIdx.x % (unsigned)NCHUNK) : 0;
  float spin = (float)threadIdx.x;
  for (int chunk = 0; chunk < NCHUNK; ++chunk) {
    const int ln = lane_recompute();
    const int c = ln & 31;
    const int hi = ln >> 5;
    const int cr = (chunk + rot) % NCHUNK;       // this chunk's id
    const int crn = (chunk + 1 + rot) % NCHUNK;  // next chunk's id
    const int buf = chunk & 1;
    const bool more = chunk + 1 < NCHUNK;
    if (more) {
      issue_w1(smem, w1, wave, crn, buf ^ 1);
      issue_w2(smem, w2, wave, crn, buf ^ 1);
    }
    if (MODE == 4) {
      // loads + ~2.5 us of pure-VALU work (no LDS, no MFMA): if the
      // DMA progresses during compute, MODE 4 ~= MODE 3; if it only
      // progresses at the wait, MODE 4 ~= MODE 3 + spin time.
#pragma unroll 4
      for (int it = 0; it < 6000; ++it) {
        spin = __builtin_fmaf(spin, 0.999f, 1.0f);
      }
      asm volatile("" :: "v"(spin));
      if (more) {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
      }
      continue;
    }
    const bf16* w1buf = &smem[OFF_W1 + buf * W1_ELEMS];
    const bf16* w2buf = &smem[OFF_W2 + buf * W2_ELEMS];

#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f32x16 acc = {};
      if (MODE == 0 || MODE == 1 || MODE == 6) {
        acc = b1_step(w1buf, af, t, c, hi);
      } else {
        asm volatile("" :: "v"(af[0]), "v"(w1buf[c]));
      }
      f32x16 st;
#pragma unroll
      for (int r = 0; r < 16; ++r) st[r] = acc[r] > 0.f ? acc[r] : 0.f;
      bf16x8 pa[2];
      t12_repack(st, pa);
      if (MODE == 0 || MODE == 2 || MODE == 6) {
        b2_step(w2buf, pa, oacc, t, c, hi);
      } else {
        asm volatile("" :: "v"(pa[0]), "v"(pa[1]), "v"(w2buf[c]));
        asm volatile("" : "+v"(oacc[0]));
      }
    }

    if (more) {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
  }

  store_tile_2b(out, oacc, m0, M, wave,
                [&](int col, size_t off, float acc) {
                  return __bfloat162float(x[off]) + alpha * (acc + b2[col]);
                });
}

}  // namespace

#ifndef DC_SAN_MAIN

at::Tensor ffn_ablate(at::Tensor x, at::Tensor w1, at::Tensor w2,
                      at::Tensor b2, double alpha, int64_t mode) {
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
  auto xp = reinterpret_cast<bf16*>(xc.data_ptr());
  auto w1p = reinterpret_cast<bf16*>(w1.data_ptr());
  auto w2p = reinterpret_cast<bf16*>(w2.data_ptr());
  auto op = reinterpret_cast<bf16*>(out.data_ptr());
  auto kern = ffn_ablate_kernel<0>;
  switch (mode) {
    case 1: kern = ffn_ablate_kernel<1>; break;
    case 2: kern = ffn_ablate_kernel<2>; break;
    case 3: kern = ffn_ablate_kernel<3>; break;
    case 4: kern = ffn_ablate_kernel<4>; break;
    case 6: kern = ffn_ablate_kernel<6>; break;
  }
  hipLaunchKernelGGL(kern, grid, block, 0, stream, xp, w1p, w2p,
                     b2c.data_ptr<float>(), op, M, (float)alpha);
  return out;
}

#endif  // DC_SAN_MAIN
