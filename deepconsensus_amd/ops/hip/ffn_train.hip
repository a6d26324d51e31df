// Training FFN pair for gfx950: fused forward and fused dgrad, both
// sequencings of the tile core in ffn_tile.h (256-row tiles, register-
// resident 2048-wide intermediate via swapped-B1 + T12 repack, glds
// double-buffered weight streaming) with fused_ffn_v3's one-shot
// prologue, chunk loop and 2-byte epilogue. This file owns what happens
// to the intermediate between B1 and B2.
//
// Reference semantics: ffn_layer.py:69-87 — h = relu(x@W1^T + b1);
// hd = dropout(h); y = hd@W2^T + b2 — and its autograd transpose.
//
//  * FWD  (MODE=0):  B1-role weights = W1 (+b1 folded in column 287),
//    ReLU + inverted dropout applied to the intermediate IN REGISTERS
//    (counter-based splitmix64 hash of (seed, element index) — no mask
//    tensor exists anywhere), hd persisted to global through the
//    T12-repacked pa fragments (16-B per-lane stores, sector-aligned),
//    B2-role weights = W2, epilogue adds b2. Returns y and hd.
//  * DGRAD (MODE=1): B1-role weights = W2^T, the combined relu x dropout
//    mask is RECOVERED from hd: hd > 0 iff (kept and h_pre > 0), so
//    dh_pre = dhd * (hd>0 ? 1/(1-p) : 0) — nothing extra was saved.
//    dh_pre is persisted (the hipBLASLt split-K wgrads x^T@dh_pre and
//    hd^T@dy consume it), B2-role weights = W1^T, no bias. Returns dx
//    and dh_pre.
//
// The wgrad GEMMs ([280,M]x[M,2048] with M >> N) stay on hipBLASLt —
// split-K shapes are the library's home turf; the fused win here is the
// two activation-shaped GEMM chains plus every elementwise between them
// (relu, dropout, mask-mul: 3 x 1.7 GB of round trips gone).

#ifndef DC_SAN_MAIN
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#endif
#include <hip/hip_runtime.h>
#include "ffn_tile.h"

namespace {

// 32-bit mix (lowbias32 family) of (seed, m row, hidden idx) -> [0,1).
// Deterministic given the host-drawn seed; statistical quality is ample
// for dropout, only the forward ever evaluates it (the backward recovers
// the mask from hd>0), and staying in 32-bit keeps the chunk loop off
// the 256-VGPR cliff (a 64-bit splitmix variant spilled 266 regs).
__device__ __forceinline__ float rand01(unsigned seed, unsigned m,
                                        unsigned h) {
  unsigned z = seed + m * 0x9E3779B9u + h * 0x85EBCA6Bu;
  z ^= z >> 16;
  z *= 0x7FEB352Du;
  z ^= z >> 15;
  z *= 0x846CA68Bu;
  z ^= z >> 16;
  return (float)(z >> 8) * (1.0f / 16777216.0f);
}

// MODE 0 = forward (relu + dropout, +b2), 1 = dgrad (mask from hread),
// 2 = dgrad WITHOUT the mask (bisection probe: dh == plain dy@W2^T).
template <int MODE>
__global__ __launch_bounds__(512, 1) void ffn_train_kernel(
    const bf16* __restrict__ x, const bf16* __restrict__ w1,
    const bf16* __restrict__ w2, const float* __restrict__ b2,
    bf16* __restrict__ out, bf16* __restrict__ hsave,
    const bf16* __restrict__ hread, int M, float p, float inv_keep,
    unsigned long long seed) {
  __shared__ __attribute__((aligned(16))) bf16 smem[LDS_ELEMS];

  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m0 = blockIdx.x * BM;

  // Stage x (FWD) / dy (DGRAD); the bias constant at col 287 is harmless
  // for DGRAD (its B1 image keeps that column zero).
  bf16x8 af[18];
  stage_x_issue_chunk0(smem, x, w1, w2, m0, M, wave, af);

  // Wave-uniform hd bases (m0, wave are SGPRs): the compiler keeps these
  // in scalar registers, so only a 32-bit per-lane offset is ever live
  // in the chunk loop — the 64-bit per-lane base this replaces was what
  // the allocator spilled (and in the dgrad instantiation its reloads
  // fed nondeterministic corruption; see profiles/r02_perf_journal.md).
  bf16* const hsave_w = hsave + (size_t)(m0 + 32 * wave) * NHID;
  const bf16* const hread_w =
      (MODE == 1) ? hread + (size_t)(m0 + 32 * wave) * NHID : nullptr;
  const int mrem = M - m0 - 32 * wave;  // lane c valid iff c < mrem

  f32x16 oacc[9] = {};

  for (int chunk = 0; chunk < NCHUNK; ++chunk) {
    const int ln = lane_recompute();
    const int c = ln & 31;
    const int hi = ln >> 5;
    const int buf = chunk & 1;
    const bool more = chunk + 1 < NCHUNK;
    if (more) {
      issue_w1(smem, w1, wave, chunk + 1, buf ^ 1);
      issue_w2(smem, w2, wave, chunk + 1, buf ^ 1);
    }
    const bf16* w1buf = &smem[OFF_W1 + buf * W1_ELEMS];
    const bf16* w2buf = &smem[OFF_W2 + buf * W2_ELEMS];

#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f32x16 acc = b1_step(w1buf, af, t, c, hi);
      __builtin_amdgcn_sched_barrier(0);  // fence: keep B1 state local
      // MFMA D-register read hazard: the cvt_pk inline asm below reads
      // acc; in MODE 0 the ~48 relu VALU ops provide the required
      // post-MFMA delay naturally, but MODE 1/2 read acc immediately
      // and measured deterministic corruption in 3 of 4 lanes (the
      // compiler's hazard recognizer does not cover asm operands
      // against the 16-pass MFMA writeback). Two s_nop 15 = 32 cycles.
      if (MODE != 0) {
        asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
      }

      // Intermediate element (m, hidden) for lane (c, hi) at index r
      // (B1 is swapped: hidden in regs, m in lanes, see b1_step):
      // m = m0 + 32*wave + c, hidden = 64*chunk + 32*t + 4*hi + (r&3)
      // + 8*(r>>2). relu/dropout applied IN-PLACE on acc (a separate
      // st[16] doubled the live range by 16 registers — the difference
      // between spilling and not).
      if (MODE == 0) {
        const int ln2 = lane_recompute();
        const unsigned mrow = m0 + 32 * wave + (ln2 & 31);
        const unsigned hbase = 64 * chunk + 32 * t + 4 * (ln2 >> 5);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float v = acc[r] > 0.f ? acc[r] : 0.f;
          if (p > 0.f) {
            const unsigned hidx = hbase + (r & 3) + 8 * (r >> 2);
            v = rand01((unsigned)seed, mrow, hidx) < p ? 0.f
                                                       : v * inv_keep;
          }
          acc[r] = v;
        }
      }
      bf16x8 pa[2];
      t12_repack(acc, pa);

      // In the repacked (B2 A-fragment) layout, lane (c, hi) holds row
      // (32*wave + c), k-span 64*chunk + 32*t + 16*s + 8*hi — so the
      // intermediate is persisted as one 16-B store per pa, and DGRAD's
      // mask read is the SAME two 16-B loads (not 16 scalar gathers in
      // the pre-repack layout, which cost 128 spilled VGPRs). Lane state
      // is re-derived fresh at each use site (unhoistable v_mbcnt) so no
      // address chain is live across an MFMA block — values that span
      // one get spilled, and their in-loop reloads carry vmcnt(0) waits
      // that drain the weight DMA queue (the v3 de-spill lesson).
      if (MODE == 1) {
        const int ln2 = lane_recompute();
        if ((ln2 & 31) < mrem) {
          const unsigned hoff = (unsigned)(ln2 & 31) * NHID + 64 * chunk
                                + 32 * t + 8 * (ln2 >> 5);
          // dh_pre = dhd * (hd>0 ? 1/(1-p) : 0), applied post-repack;
          // one h fragment live at a time.
          {
            const bf16x8 h0 =
                *reinterpret_cast<const bf16x8*>(hread_w + hoff);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              pa[0][j] = (float)h0[j] > 0.f
                             ? (__bf16)((float)pa[0][j] * inv_keep)
                             : (__bf16)0.f;
            }
          }
          {
            const bf16x8 h1 =
                *reinterpret_cast<const bf16x8*>(hread_w + hoff + 16);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              pa[1][j] = (float)h1[j] > 0.f
                             ? (__bf16)((float)pa[1][j] * inv_keep)
                             : (__bf16)0.f;
            }
          }
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            pa[0][j] = (__bf16)0.f;
            pa[1][j] = (__bf16)0.f;
          }
        }
      }

      __builtin_amdgcn_sched_barrier(0);  // fence: mask/repack local
      // Persist the intermediate before B2 (pa dies at its last B2
      // use instead of staying live across all 18 MFMAs for a post-B2
      // store — the difference between 0 and ~8 spilled VGPRs here).
      {
        const int ln2 = lane_recompute();
        if ((ln2 & 31) < mrem) {
          const unsigned hoff = (unsigned)(ln2 & 31) * NHID + 64 * chunk
                                + 32 * t + 8 * (ln2 >> 5);
          *reinterpret_cast<bf16x8*>(hsave_w + hoff) = pa[0];
          *reinterpret_cast<bf16x8*>(hsave_w + hoff + 16) = pa[1];
        }
      }

      __builtin_amdgcn_sched_barrier(0);  // fence: store addrs die here
      b2_step(w2buf, pa, oacc, t, c, hi);
    }

    if (more) {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
  }

  // Epilogue: plain y (+b2 in FWD); the ReZero residual/post-dropout
  // stay in the wrapper (they are part of its autograd graph).
  store_tile_2b(out, oacc, m0, M, wave,
                [&](int col, size_t, float acc) {
                  return acc + ((MODE == 0) ? b2[col] : 0.f);
                });
}

}  // namespace

#ifndef DC_SAN_MAIN

std::vector<at::Tensor> ffn_train_fwd(at::Tensor x, at::Tensor w1,
                                      at::Tensor w2, at::Tensor b2,
                                      double p_drop, int64_t seed) {
  TORCH_CHECK(x.is_cuda() && x.dtype() == at::kBFloat16,
              "x must be bf16 on device");
  auto xc = x.contiguous();
  const int K = xc.size(-1);
  const int M = xc.numel() / K;
  TORCH_CHECK(K == K1, "ffn_train_fwd requires width 280");
  TORCH_CHECK((int64_t)M * NHID < (1ll << 31),
              "ffn_train_fwd: M too large for 32-bit hd offsets");
  TORCH_CHECK(w1.size(0) == NHID && w1.size(1) == K1P,
              "w1 must be [2048, 296] with b1 folded into column 287");
  TORCH_CHECK(w2.size(0) == 320 && w2.size(1) == NHID,
              "w2 must be padded [320, 2048]");
  auto b2c = b2.contiguous();
  TORCH_CHECK(b2c.dtype() == at::kFloat && b2c.numel() >= NOUT,
              "b2 must be fp32 [280]");
  auto y = at::empty({M, K1}, xc.options());
  auto hd = at::empty({M, NHID}, xc.options());
  const float p = (float)p_drop;
  dim3 grid((M + BM - 1) / BM);
  hipStream_t stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(ffn_train_kernel<0>, grid, dim3(512), 0, stream,
                     reinterpret_cast<bf16*>(xc.data_ptr()),
                     reinterpret_cast<bf16*>(w1.data_ptr()),
                     reinterpret_cast<bf16*>(w2.data_ptr()),
                     b2c.data_ptr<float>(),
                     reinterpret_cast<bf16*>(y.data_ptr()),
                     reinterpret_cast<bf16*>(hd.data_ptr()), nullptr, M, p,
                     p < 1.f ? 1.f / (1.f - p) : 0.f,
                     (unsigned long long)seed);
  return {y, hd};
}

std::vector<at::Tensor> ffn_train_dgrad_impl(at::Tensor dy, at::Tensor hd,
                                             at::Tensor w2t, at::Tensor w1t,
                                             double p_drop, bool nomask);

std::vector<at::Tensor> ffn_train_dgrad(at::Tensor dy, at::Tensor hd,
                                        at::Tensor w2t, at::Tensor w1t,
                                        double p_drop) {
  return ffn_train_dgrad_impl(dy, hd, w2t, w1t, p_drop, false);
}

std::vector<at::Tensor> ffn_train_dgrad_nomask(at::Tensor dy, at::Tensor hd,
                                               at::Tensor w2t,
                                               at::Tensor w1t,
                                               double p_drop) {
  return ffn_train_dgrad_impl(dy, hd, w2t, w1t, p_drop, true);
}

std::vector<at::Tensor> ffn_train_dgrad_impl(at::Tensor dy, at::Tensor hd,
                                             at::Tensor w2t, at::Tensor w1t,
                                             double p_drop, bool nomask) {
  TORCH_CHECK(dy.is_cuda() && dy.dtype() == at::kBFloat16,
              "dy must be bf16 on device");
  auto dyc = dy.contiguous();
  const int K = dyc.size(-1);
  const int M = dyc.numel() / K;
  TORCH_CHECK(K == K1, "ffn_train_dgrad requires width 280");
  TORCH_CHECK((int64_t)M * NHID < (1ll << 31),
              "ffn_train_dgrad: M too large for 32-bit hd offsets");
  TORCH_CHECK(w2t.size(0) == NHID && w2t.size(1) == K1P,
              "w2t must be [2048, 296] (W2^T image, column 287 zero)");
  TORCH_CHECK(w1t.size(0) == 320 && w1t.size(1) == NHID,
              "w1t must be padded [320, 2048] (W1^T image)");
  auto hdc = hd.contiguous();
  TORCH_CHECK(hdc.dtype() == at::kBFloat16 &&
                  hdc.numel() == (int64_t)M * NHID,
              "hd must be bf16 [M, 2048]");
  auto dx = at::empty({M, K1}, dyc.options());
  auto dh = at::empty({M, NHID}, dyc.options());
  const float p = (float)p_drop;
  dim3 grid((M + BM - 1) / BM);
  hipStream_t stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(nomask ? ffn_train_kernel<2> : ffn_train_kernel<1>,
                     grid, dim3(512), 0, stream,
                     reinterpret_cast<bf16*>(dyc.data_ptr()),
                     reinterpret_cast<bf16*>(w2t.data_ptr()),
                     reinterpret_cast<bf16*>(w1t.data_ptr()), nullptr,
                     reinterpret_cast<bf16*>(dx.data_ptr()),
                     reinterpret_cast<bf16*>(dh.data_ptr()),
                     reinterpret_cast<bf16*>(hdc.data_ptr()), M, p,
                     p < 1.f ? 1.f / (1.f - p) : 0.f, 0ull);
  return {dx, dh};
}

#endif  // DC_SAN_MAIN
