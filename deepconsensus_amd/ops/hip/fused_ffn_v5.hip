// Fused FFN v5 for gfx950: the tile core of ffn_tile.h inside a persistent
// grid, with the per-tile work around the chunk loop removed or overlapped.
//
// Same math, weight layouts and accumulation order as fused_ffn_v3.hip
// (W1 [2048, 296] with b1 in column 287, W2 padded [320, 2048], fp32 b2):
// both kernels run the same shared B1 / repack / B2 steps per chunk, so the
// two agree bitwise. What this kernel owns is everything a one-shot v3
// block pays serially per 256-row tile:
//  * persistent grid: one block per CU walks tiles blockIdx.x, +gridDim.x,
//    ... instead of ~25 launch/drain rounds of one-shot blocks;
//  * continuous weight stream: the double-buffered glds rotation runs
//    across tile boundaries. NCHUNK is even, so chunk 0 always lives in
//    buffer 0: during chunk 31 of a tile, chunk 0 of the next tile is
//    issued into buffer 0 under the same wait + barrier as every other
//    chunk. Only a block's first tile pays a cold chunk 0;
//  * no LDS staging of x: each lane loads its 18 A-fragments (16
//    contiguous bytes of its own row each) straight from global, as
//    fused_condense does. Fragment 17 is built in registers: columns
//    272-279 from memory, 280-286 zero, 287 = bf16(1.0) for in-range rows
//    (the constant-1 column that multiplies the folded b1);
//  * epilogue: when the loop ends buffer 1 of W1 and W2 is idle (the next
//    tile's chunk 0 sits in buffer 0), so each wave transposes its oacc
//    through a private slice of it, 8 rows at a time, and reads the
//    residual / writes out with 16-B accesses instead of 2-B ones.

#ifndef DC_SAN_MAIN
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#endif
#include <hip/hip_runtime.h>
#include "ffn_tile.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// Epilogue transpose slices: one eighth of W1[1] and of W2[1] per wave,
// each holding 4 fp32 output rows (4 x 1,120 B).
constexpr int EPI_A = W1_ELEMS / 8;  // 2,368 elems = 4,736 B
constexpr int EPI_B = W2_ELEMS / 8;  // 2,592 elems = 5,184 B
constexpr int NQ = NOUT / 8;         // 35 16-B output granules per row
constexpr int EPI_ITERS = (8 * NQ + 63) / 64;  // 8 rows x 35 over 64 lanes
static_assert(NCHUNK % 2 == 0, "chunk 0 must land in buffer 0 every tile");
static_assert(EPI_A * 2 >= 4 * NOUT * 4 && EPI_B * 2 >= 4 * NOUT * 4,
              "a slice holds 4 fp32 rows");
static_assert((EPI_A * 2) % 16 == 0 && (EPI_B * 2) % 16 == 0,
              "slices stay 16-B aligned");

__device__ __forceinline__ float bf16_lo(unsigned w) {
  return __uint_as_float(w << 16);
}
__device__ __forceinline__ float bf16_hi(unsigned w) {
  return __uint_as_float(w & 0xffff0000u);
}
__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {
  return (unsigned)__bfloat16_as_ushort(__float2bfloat16(lo)) |
         ((unsigned)__bfloat16_as_ushort(__float2bfloat16(hi)) << 16);
}

__global__ __launch_bounds__(512, 1) void fused_ffn_v5_kernel(
    const bf16* __restrict__ x, const bf16* __restrict__ w1,
    const bf16* __restrict__ w2, const float* __restrict__ b2,
    bf16* __restrict__ out, int M, float alpha, int num_tiles) {
  __shared__ __attribute__((aligned(16))) bf16 smem[LDS_ELEMS];

  // wave id lives in an SGPR (readfirstlane) — free to keep live.
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

  // The only cold chunk 0 of this block; every later tile finds its
  // chunk 0 issued during the previous tile's last chunk.
  issue_w1(smem, w1, wave, 0, 0);
  issue_w2(smem, w2, wave, 0, 0);

  for (int tile = blockIdx.x; tile < num_tiles; tile += gridDim.x) {
    const int m0 = tile * BM;
    const bool has_next = tile + (int)gridDim.x < num_tiles;

    // ---- A-fragments straight from global: lane (c, hi) of wave w owns
    // row m0 + 32w + c, columns 16s + 8hi .. +7. Rows at or beyond M give
    // zero fragments, bias column included. No LDS image of x exists, so
    // v3's hazard of a chunk-1 glds overwriting the staging region under
    // in-flight af ds_reads is gone, and with it the wait that guarded
    // it. ----
    bf16x8 af[18];
    {
      const int ln = lane_recompute();
      const int c = ln & 31;
      const int hi = ln >> 5;
      const int row = m0 + 32 * wave + c;
      if (row < M) {
        const bf16* xr = x + (size_t)row * K1 + 8 * hi;
#pragma unroll
        for (int s = 0; s < 17; ++s) {
          af[s] = *reinterpret_cast<const bf16x8*>(xr + 16 * s);
        }
        if (hi == 0) {
          af[17] = *reinterpret_cast<const bf16x8*>(xr + 16 * 17);
        } else {
          // cols 280..286 zero, col 287 = bf16(1.0) (upper half of .w)
          af[17] = __builtin_bit_cast(bf16x8, u32x4{0u, 0u, 0u, 0x3f800000u});
        }
      } else {
#pragma unroll
        for (int s = 0; s < 18; ++s) af[s] = bf16x8{};
      }
    }

    // Tile-top barrier. It orders two things:
    //  (a) first tile: every wave's share of the cold chunk 0 has landed
    //      (vmcnt(0)) before any wave reads buffer 0;
    //  (b) later tiles: every wave has finished the epilogue ds_reads of
    //      its buffer-1 slice (lgkmcnt(0) — a raw s_barrier drains
    //      nothing) before chunk 0 below issues chunk 1's glds into
    //      buffer 1.
    // vmcnt(0) also retires this tile's af loads before the first MFMA.
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    f32x16 oacc[9] = {};

    for (int chunk = 0; chunk < NCHUNK; ++chunk) {
      const int ln = lane_recompute();
      const int c = ln & 31;   // loop-local, dead at the backedge ->
      const int hi = ln >> 5;  // nothing to spill
      const int buf = chunk & 1;
      // The rotation does not stop at the tile boundary: the last chunk
      // issues the next tile's chunk 0 into buffer 0 (= buf ^ 1).
      const int nxt = (chunk + 1) & (NCHUNK - 1);
      if (chunk + 1 < NCHUNK || has_next) {
        issue_w1(smem, w1, wave, nxt, buf ^ 1);
        issue_w2(smem, w2, wave, nxt, buf ^ 1);
      }
      const bf16* w1buf = &smem[OFF_W1 + buf * W1_ELEMS];
      const bf16* w2buf = &smem[OFF_W2 + buf * W2_ELEMS];

      // Per 32-hidden tile: B1, ReLU, repack, then its two B2 k-steps —
      // v3's sequence of the shared steps.
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

      // The DMA groups issued above must have landed and every wave must
      // be done reading buffer `buf`. After the last chunk this is also
      // what frees buffer 1 for the epilogue slices below (and lands the
      // next tile's chunk 0), so unlike v3 it runs on every chunk.
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }

    // ---- Epilogue: b2 + ReZero alpha + residual. Each wave moves its
    // 32 x 280 fp32 (oacc + b2) through its private slices of the idle
    // buffer 1, 8 rows per pass: D registers 4g..4g+3 are rows 8g + j
    // (hi = 0, slice of W1[1]) and 8g + 4 + j (hi = 1, slice of W2[1]).
    // Lanes then walk the 8 x 35 16-B granules of the pass row-major: two
    // ds_read_b128, one 16-B residual load, one 16-B store. Only this
    // wave touches its slices, and a wave's LDS ops execute in order, so
    // lgkmcnt waits are all the ordering the passes need. ----
    {
      const int lne = lane_recompute();
      const int ce = lne & 31;
      const int hie = lne >> 5;
      float* slice_a =
          reinterpret_cast<float*>(&smem[OFF_W1 + W1_ELEMS + wave * EPI_A]);
      float* slice_b =
          reinterpret_cast<float*>(&smem[OFF_W2 + W2_ELEMS + wave * EPI_B]);
      float* slice_w = hie ? slice_b : slice_a;
      // b2 is read once, ahead of the residual: a per-pass reload would
      // put a vmcnt(0) (= drain of the out stores) into every pass.
      float bias[9];
#pragma unroll
      for (int ct = 0; ct < 9; ++ct) bias[ct] = b2[min(32 * ct + ce, NOUT - 1)];
      // All of this lane's residual granules are requested before its
      // first out store, so no residual wait ever has to drain a store:
      // three passes up front (af is dead, the registers are there), the
      // fourth once pass 0's LDS writes have freed a quarter of oacc. The
      // loads are unconditional (row and granule clamped in range, the
      // store is what is masked) so they carry no divergent branch and
      // the load latency is exposed once per tile.
      u32x4 rv[4][EPI_ITERS];
      auto load_resid = [&](int g) {
#pragma unroll
        for (int it = 0; it < EPI_ITERS; ++it) {
          const int idx = min(it * 64 + lne, 8 * NQ - 1);
          const int row = min(m0 + 32 * wave + 8 * g + idx / NQ, M - 1);
          rv[g][it] = *reinterpret_cast<const u32x4*>(
              x + (size_t)row * K1 + 8 * (idx % NQ));
        }
      };
      load_resid(0);
      load_resid(1);
      load_resid(2);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
#pragma unroll
        for (int ct = 0; ct < 9; ++ct) {
          const int col = 32 * ct + ce;
          if (col < NOUT) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              slice_w[j * NOUT + col] = oacc[ct][4 * g + j] + bias[ct];
            }
          }
        }
        if (g == 0) load_resid(3);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int it = 0; it < EPI_ITERS; ++it) {
          const int idx = it * 64 + lne;
          const int rl = idx / NQ, q = idx % NQ;
          const int row = m0 + 32 * wave + 8 * g + rl;
          if (idx < 8 * NQ && row < M) {
            const float* src =
                (rl < 4 ? slice_a + rl * NOUT : slice_b + (rl - 4) * NOUT) +
                8 * q;
            const f32x4 t0 = *reinterpret_cast<const f32x4*>(src);
            const f32x4 t1 = *reinterpret_cast<const f32x4*>(src + 4);
            const u32x4 r = rv[g][it];
            u32x4 ov;
            ov.x = pack_bf16(bf16_lo(r.x) + alpha * t0.x,
                             bf16_hi(r.x) + alpha * t0.y);
            ov.y = pack_bf16(bf16_lo(r.y) + alpha * t0.z,
                             bf16_hi(r.y) + alpha * t0.w);
            ov.z = pack_bf16(bf16_lo(r.z) + alpha * t1.x,
                             bf16_hi(r.z) + alpha * t1.y);
            ov.w = pack_bf16(bf16_lo(r.w) + alpha * t1.z,
                             bf16_hi(r.w) + alpha * t1.w);
            *reinterpret_cast<u32x4*>(out + (size_t)row * K1 + 8 * q) = ov;
          }
        }
        // This pass's slice reads retire before the next pass (or, via
        // the tile-top barrier, another wave's glds) rewrites the slice.
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
    }
  }
}

}  // namespace

#ifndef DC_SAN_MAIN

at::Tensor fused_ffn_v5(at::Tensor x, at::Tensor w1, at::Tensor w2,
                        at::Tensor b2, double alpha, int64_t max_blocks) {
  TORCH_CHECK(x.is_cuda() && x.dtype() == at::kBFloat16,
              "x must be bf16 on device");
  auto xc = x.contiguous();
  const int K = xc.size(-1);
  const int M = xc.numel() / K;
  TORCH_CHECK(K == K1, "fused_ffn_v5 requires width 280");
  TORCH_CHECK(w1.size(0) == NHID && w1.size(1) == K1P,
              "w1 must be [2048, 296] with b1 folded into column 287");
  TORCH_CHECK(w2.size(0) == 320 && w2.size(1) == NHID,
              "w2 must be padded [320, 2048]");
  TORCH_CHECK(b2.numel() >= NOUT, "b2 must cover 280 outputs");
  TORCH_CHECK(max_blocks >= 0, "max_blocks must be >= 0 (0 = one per CU)");
  auto b2c = b2.contiguous();
  TORCH_CHECK(b2c.dtype() == at::kFloat, "b2 must be fp32");
  auto out = at::empty_like(xc);
  const int num_tiles = (M + BM - 1) / BM;
  if (num_tiles == 0) return out;
  // Persistent grid: 160,768 B of LDS = one resident block per CU.
  const int64_t cap =
      max_blocks > 0
          ? max_blocks
          : at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  dim3 grid((unsigned)std::min<int64_t>(num_tiles, cap));
  dim3 block(512);
  hipStream_t stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(fused_ffn_v5_kernel, grid, block, 0, stream,
                     reinterpret_cast<bf16*>(xc.data_ptr()),
                     reinterpret_cast<bf16*>(w1.data_ptr()),
                     reinterpret_cast<bf16*>(w2.data_ptr()),
                     b2c.data_ptr<float>(),
                     reinterpret_cast<bf16*>(out.data_ptr()), M,
                     (float)alpha, num_tiles);
  return out;
}

#endif  // DC_SAN_MAIN
