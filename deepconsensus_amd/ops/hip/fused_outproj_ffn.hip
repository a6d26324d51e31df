// Attention out-projection folded into the persistent FFN for gfx950:
// fused_ffn_v5 (persistent grid, continuous weight stream, 16-B epilogue)
// with a per-tile prologue in place of v5's "A-fragments straight from
// global" block. The prologue computes
//   flat = resid + alpha_attn * bf16(a @ Wout^T)
// for this wave's 32 rows directly into the FFN's A-fragments af[18], so
// the fused_linear launch that produced `flat`, its [M, 280] write and the
// FFN's A-fragment read of it are gone.
//
// The out-projection has the operand shapes of a sixth of one B1 GEMM:
// wout_pad [320, 296] is five [64, 296] images in the layout of one W1
// chunk, b1_step gives "32 weight rows x this wave's 32 input rows", and
// t12_repack turns its D registers into two A-fragments in exactly the
// af[] layout (lane (c, hi): row c, columns 16s + 8hi .. +7). Nine 32-row
// tiles T0..T8 of Wout (output columns 0..287; rows 280+ are zero) build
// af[0..17]. The same (a, w) pairs are multiplied in the same k-step order
// as in fused_linear, the accumulator is rounded to bf16 first and the
// residual applied as bf16(float(res) + alpha * float(v)), as there.
//
// The finished fragments are also stored to `mid` [M, 280]: the v5
// epilogue reads its residual from there, unchanged. Those reads come from
// the wave that stored the rows, >= 32 vmcnt(0) + barrier phases later,
// from addresses this CU has not read before.
//
// LDS rotation (W1[b] / W2[b] = buffer b of the two regions; a Wout chunk
// of 37,888 B fits either). FFN chunk 0 must sit in buffer 0 of both
// regions when the chunk loop starts, and the epilogue's per-wave slices
// occupy buffer 1 of both regions until the tile-top barrier. Every phase
// ends in s_waitcnt vmcnt(0) lgkmcnt(0) + s_barrier (a raw barrier drains
// nothing), which both lands the phase's DMA and frees what it read:
//
//   phase      reads               issues (glds)
//   chunk 31   W1[1], W2[1]        next tile: Wout0 -> W1[0], Wout1 -> W2[0]
//   epilogue   slices of buffer 1  -
//   tile top   -                   (a fragments, residual fragments of A)
//   A  T0..T3  W1[0], W2[0]        Wout2 -> W1[1], Wout3 -> W2[1]
//   B  T4, T5  W1[1]               FFN W1 chunk 0 -> W1[0]
//   C  T6, T7  W2[1]               Wout4 rows 0..31 -> W1[1]; FFN W2 chunk 0
//                                  -> W2[0]
//   D  T8      W1[1]               -
//   chunk 0    W1[0], W2[0]        chunk 1 -> buffer 1, as in v5
//
// so only a block's first tile pays a cold Wout0/Wout1. Residual fragments
// are requested one phase ahead, before that phase's glds issues: vmcnt
// retires in order, so a load issued behind the DMA would wait for it.
//
// The chunk loop is v5's; its only difference is what the last chunk
// prefetches for the next tile.

#ifndef DC_SAN_MAIN
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#endif
#include <hip/hip_runtime.h>
#include "ffn_tile.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// Epilogue transpose slices, as in fused_ffn_v5.hip.
constexpr int EPI_A = W1_ELEMS / 8;  // 2,368 elems = 4,736 B
constexpr int EPI_B = W2_ELEMS / 8;  // 2,592 elems = 5,184 B
constexpr int NQ = NOUT / 8;         // 35 16-B output granules per row
constexpr int EPI_ITERS = (8 * NQ + 63) / 64;  // 8 rows x 35 over 64 lanes
// Wout tile T8 = the first 32 rows of chunk 4: 18,944 B -> 19 1-KiB pieces
// (the last one runs 512 B into row 32; source and destination both have
// the room).
constexpr int WOUT_HALF_CHUNKS = (32 * K1P * 2 + 1023) / 1024;
static_assert(NCHUNK % 2 == 0, "chunk 0 must land in buffer 0 every tile");
static_assert(W2_ELEMS >= W1_ELEMS, "a Wout chunk fits a W2 buffer");
static_assert(WOUT_HALF_CHUNKS * 512 <= W1_ELEMS, "T8 fits W1[1]");
static_assert(4 * W1_ELEMS + WOUT_HALF_CHUNKS * 512 <= 320 * K1P,
              "T8's pieces stay inside wout_pad");
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

// Wout chunk `chunk` ([64, 296] raw image, the first NCK 1-KiB pieces of
// it) to LDS element offset dst_base. Same shape as issue_w1, readfirstlane
// on the destination included (see its comment in ffn_tile.h).
template <int NCK>
__device__ __forceinline__ void issue_wout(bf16* smem, const bf16* wout,
                                           int wave, int chunk,
                                           int dst_base) {
  const int ln = lane_recompute();
  const bf16* src = wout + (size_t)chunk * W1_ELEMS;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int ck = wave + i * 8;
    if (ck < NCK) {
      const int dst_off =
          __builtin_amdgcn_readfirstlane(dst_base + ck * 512);
      glds16(src + ck * 512 + ln * 8, &smem[dst_off]);
    }
  }
}

// Residual fragments F0 .. F1-1 of this lane's row (rr = resid + row * 280
// + 8 * hi). Rows at or beyond M and columns at or beyond 280 (fragment 17,
// hi = 1) are never read and stay zero.
template <int F0, int F1>
__device__ __forceinline__ void load_resid_frags(bf16x8 (&rs)[18],
                                                 const bf16* rr, bool row_ok,
                                                 int hi) {
#pragma unroll
  for (int f = F0; f < F1; ++f) {
    rs[f] = bf16x8{};
    if (row_ok && (f < 17 || hi == 0)) {
      rs[f] = *reinterpret_cast<const bf16x8*>(rr + 16 * f);
    }
  }
}

// Out-projection tile T9 (output columns 32*T9 .. +31) from the Wout chunk
// image at wbuf: 18 swapped MFMAs, repack, residual; the two finished
// fragments go to af[2*T9], af[2*T9 + 1] and to `mid` (mr = mid + row * 280
// + 8 * hi).
template <int T9>
__device__ __forceinline__ void outproj_tile(const bf16* wbuf,
                                             const bf16x8 (&aa)[18],
                                             const bf16x8 (&rs)[18],
                                             bf16x8 (&af)[18], bf16* mr,
                                             bool row_ok, float alpha, int c,
                                             int hi) {
  f32x16 acc = b1_step(wbuf, aa, T9 & 1, c, hi);
  // fused_linear adds its (absent, 0.f) bias before rounding: keeps -0 -> +0.
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = acc[r] + 0.f;
  bf16x8 pa[2];
  t12_repack(acc, pa);
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const bf16x8 res = rs[2 * T9 + s];
    bf16x8 v = pa[s];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float rv = (float)res[j];
      const float vv = (float)v[j];
      v[j] = (__bf16)(rv + alpha * vv);
    }
    if (2 * T9 + s == 17 && hi == 1) {
      // cols 280..286 zero, col 287 = bf16(1.0) (upper half of .w) for
      // in-range rows: the constant-1 column that multiplies the folded b1.
      v = __builtin_bit_cast(
          bf16x8, u32x4{0u, 0u, 0u, row_ok ? 0x3f800000u : 0u});
    } else if (row_ok) {
      *reinterpret_cast<bf16x8*>(mr + 16 * (2 * T9 + s)) = v;
    }
    af[2 * T9 + s] = v;
  }
}

__global__ __launch_bounds__(512, 1) void fused_outproj_ffn_kernel(
    const bf16* __restrict__ a, const bf16* __restrict__ resid,
    const bf16* __restrict__ wout, const bf16* __restrict__ w1,
    const bf16* __restrict__ w2, const float* __restrict__ b2, bf16* mid,
    bf16* __restrict__ out, int M, float alpha_attn, float alpha, int num_tiles) {
  __shared__ __attribute__((aligned(16))) bf16 smem[LDS_ELEMS];

  // wave id lives in an SGPR (readfirstlane) — free to keep live.
  const int wave0 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

  // The only cold Wout0/Wout1 of this block; every later tile finds them
  // issued during the previous tile's last chunk.
  issue_wout<W1_CHUNKS>(smem, wout, wave0, 0, OFF_W1);
  issue_wout<W1_CHUNKS>(smem, wout, wave0, 1, OFF_W2);

  for (int tile = blockIdx.x; tile < num_tiles; tile += gridDim.x) {
    const int m0 = tile * BM;
    const bool has_next = tile + (int)gridDim.x < num_tiles;
    // Opaque per tile: otherwise the prologue's ~30 wave-derived DMA
    // source and destination scalars are hoisted out of the tile loop,
    // outnumber the SGPRs and get spilled.
    int wave = wave0;
    asm volatile("" : "+s"(wave));

    // ---- Prologue: af = resid + alpha_attn * bf16(a @ Wout^T) for this
    // wave's rows, in the FFN's A-fragment layout. Lane (c, hi) of wave w
    // owns row m0 + 32w + c, columns 16s + 8hi .. +7 of a, resid, mid and
    // af alike. Rows at or beyond M give zero fragments, bias column
    // included. All lane state here is dead at the chunk loop. ----
    bf16x8 af[18];
    {
      const int ln = lane_recompute();
      const int c = ln & 31;
      const int hi = ln >> 5;
      const int row = m0 + 32 * wave + c;
      const bool row_ok = row < M;
      const size_t roff = (size_t)(row_ok ? row : 0) * K1 + 8 * hi;
      const bf16* rr = resid + roff;
      bf16* mr = mid + roff;

      bf16x8 aa[18];
      bf16x8 rs[18];
      if (row_ok) {
        const bf16* ar = a + roff;
#pragma unroll
        for (int s = 0; s < 17; ++s) {
          aa[s] = *reinterpret_cast<const bf16x8*>(ar + 16 * s);
        }
        // cols 280..287 of a do not exist: zero, and no bias column.
        aa[17] = bf16x8{};
        if (hi == 0) aa[17] = *reinterpret_cast<const bf16x8*>(ar + 16 * 17);
      } else {
#pragma unroll
        for (int s = 0; s < 18; ++s) aa[s] = bf16x8{};
      }
      load_resid_frags<0, 8>(rs, rr, row_ok, hi);

      // Tile-top barrier. It orders two things:
      //  (a) first tile: every wave's share of the cold Wout0/Wout1 has
      //      landed (vmcnt(0)) before any wave reads buffer 0;
      //  (b) later tiles: every wave has finished the epilogue ds_reads of
      //      its buffer-1 slice (lgkmcnt(0)) before phase A issues
      //      Wout2/Wout3 into buffer 1.
      // vmcnt(0) also retires this tile's a loads before the first MFMA.
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();

      // Phase A: T0..T3 from buffer 0; Wout2/Wout3 into buffer 1.
      load_resid_frags<8, 12>(rs, rr, row_ok, hi);
      issue_wout<W1_CHUNKS>(smem, wout, wave, 2, OFF_W1 + W1_ELEMS);
      issue_wout<W1_CHUNKS>(smem, wout, wave, 3, OFF_W2 + W2_ELEMS);
      outproj_tile<0>(&smem[OFF_W1], aa, rs, af, mr, row_ok, alpha_attn, c,
                      hi);
      outproj_tile<1>(&smem[OFF_W1], aa, rs, af, mr, row_ok, alpha_attn, c,
                      hi);
      outproj_tile<2>(&smem[OFF_W2], aa, rs, af, mr, row_ok, alpha_attn, c,
                      hi);
      outproj_tile<3>(&smem[OFF_W2], aa, rs, af, mr, row_ok, alpha_attn, c,
                      hi);
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();

      // Phase B: T4, T5 from W1[1]; buffer 0 is free -> FFN W1 chunk 0.
      load_resid_frags<12, 16>(rs, rr, row_ok, hi);
      issue_w1(smem, w1, wave, 0, 0);
      outproj_tile<4>(&smem[OFF_W1 + W1_ELEMS], aa, rs, af, mr, row_ok,
                      alpha_attn, c, hi);
      outproj_tile<5>(&smem[OFF_W1 + W1_ELEMS], aa, rs, af, mr, row_ok,
                      alpha_attn, c, hi);
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();

      // Phase C: T6, T7 from W2[1]; W1[1] is free -> T8's half chunk;
      // FFN W2 chunk 0 -> W2[0].
      load_resid_frags<16, 18>(rs, rr, row_ok, hi);
      issue_wout<WOUT_HALF_CHUNKS>(smem, wout, wave, 4, OFF_W1 + W1_ELEMS);
      issue_w2(smem, w2, wave, 0, 0);
      outproj_tile<6>(&smem[OFF_W2 + W2_ELEMS], aa, rs, af, mr, row_ok,
                      alpha_attn, c, hi);
      outproj_tile<7>(&smem[OFF_W2 + W2_ELEMS], aa, rs, af, mr, row_ok,
                      alpha_attn, c, hi);
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();

      // Phase D: T8 from W1[1]. Its barrier frees buffer 1 for the chunk-1
      // glds that chunk 0 issues; vmcnt(0) retires the mid stores.
      outproj_tile<8>(&smem[OFF_W1 + W1_ELEMS], aa, rs, af, mr, row_ok,
                      alpha_attn, c, hi);
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }

    f32x16 oacc[9] = {};

    for (int chunk = 0; chunk < NCHUNK; ++chunk) {
      const int ln = lane_recompute();
      const int c = ln & 31;   // loop-local, dead at the backedge ->
      const int hi = ln >> 5;  // nothing to spill
      const int buf = chunk & 1;
      // The rotation does not stop at the tile boundary: the last chunk
      // issues the next tile's Wout0/Wout1 into buffer 0 (= buf ^ 1).
      if (chunk + 1 < NCHUNK) {
        issue_w1(smem, w1, wave, chunk + 1, buf ^ 1);
        issue_w2(smem, w2, wave, chunk + 1, buf ^ 1);
      } else if (has_next) {
        issue_wout<W1_CHUNKS>(smem, wout, wave, 0, OFF_W1);
        issue_wout<W1_CHUNKS>(smem, wout, wave, 1, OFF_W2);
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
      // next tile's Wout0/Wout1).
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }

    // ---- Epilogue: b2 + ReZero alpha + residual, v5's, with the residual
    // read from `mid` (this wave's own prologue stores, retired by every
    // vmcnt(0) since). Each wave moves its 32 x 280 fp32 (oacc + b2)
    // through its private slices of the idle buffer 1, 8 rows per pass: D
    // registers 4g..4g+3 are rows 8g + j (hi = 0, slice of W1[1]) and
    // 8g + 4 + j (hi = 1, slice of W2[1]). Lanes then walk the 8 x 35 16-B
    // granules of the pass row-major: two ds_read_b128, one 16-B residual
    // load, one 16-B store. Only this wave touches its slices, and a
    // wave's LDS ops execute in order, so lgkmcnt waits are all the
    // ordering the passes need. ----
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
              mid + (size_t)row * K1 + 8 * (idx % NQ));
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

at::Tensor fused_outproj_ffn(at::Tensor a, at::Tensor resid,
                             at::Tensor wout, double alpha_attn,
                             at::Tensor w1, at::Tensor w2, at::Tensor b2,
                             double alpha_ffn, int64_t max_blocks) {
  TORCH_CHECK(a.is_cuda() && a.dtype() == at::kBFloat16,
              "a must be bf16 on device");
  TORCH_CHECK(resid.is_cuda() && resid.dtype() == at::kBFloat16,
              "resid must be bf16 on device");
  auto ac = a.contiguous();
  auto rc = resid.contiguous();
  const int K = ac.size(-1);
  const int M = ac.numel() / K;
  TORCH_CHECK(K == K1, "fused_outproj_ffn requires width 280");
  TORCH_CHECK(rc.numel() == ac.numel(), "resid must match a");
  // The kernel streams the weights as raw row-major bf16 images straight
  // from their data pointers: layouts are checked, not fixed up.
  TORCH_CHECK(wout.is_cuda() && wout.dtype() == at::kBFloat16 &&
                  wout.dim() == 2 && wout.is_contiguous() &&
                  wout.size(0) == 320 && wout.size(1) == K1P,
              "wout must be contiguous bf16 [320, 296]");
  TORCH_CHECK(w1.is_cuda() && w1.dtype() == at::kBFloat16 &&
                  w1.is_contiguous() && w1.dim() == 2 &&
                  w1.size(0) == NHID && w1.size(1) == K1P,
              "w1 must be [2048, 296] with b1 folded into column 287");
  TORCH_CHECK(w2.is_cuda() && w2.dtype() == at::kBFloat16 &&
                  w2.is_contiguous() && w2.dim() == 2 &&
                  w2.size(0) == 320 && w2.size(1) == NHID,
              "w2 must be padded [320, 2048]");
  TORCH_CHECK(b2.numel() >= NOUT, "b2 must cover 280 outputs");
  TORCH_CHECK(max_blocks >= 0, "max_blocks must be >= 0 (0 = one per CU)");
  auto b2c = b2.contiguous();
  TORCH_CHECK(b2c.is_cuda() && b2c.dtype() == at::kFloat, "b2 must be fp32");
  auto out = at::empty({M, K1}, ac.options());
  const int num_tiles = (M + BM - 1) / BM;
  if (num_tiles == 0) return out;
  // The post-attention activations: written by the prologue, read back by
  // the epilogue as its residual.
  auto mid = at::empty({M, K1}, ac.options());
  // Persistent grid: 160,768 B of LDS = one resident block per CU.
  const int64_t cap =
      max_blocks > 0
          ? max_blocks
          : at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  dim3 grid((unsigned)std::min<int64_t>(num_tiles, cap));
  dim3 block(512);
  hipStream_t stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(fused_outproj_ffn_kernel, grid, block, 0, stream,
                     reinterpret_cast<bf16*>(ac.data_ptr()),
                     reinterpret_cast<bf16*>(rc.data_ptr()),
                     reinterpret_cast<bf16*>(wout.data_ptr()),
                     reinterpret_cast<bf16*>(w1.data_ptr()),
                     reinterpret_cast<bf16*>(w2.data_ptr()),
                     b2c.data_ptr<float>(),
                     reinterpret_cast<bf16*>(mid.data_ptr()),
                     reinterpret_cast<bf16*>(out.data_ptr()), M,
                     (float)alpha_attn, (float)alpha_ffn, num_tiles);
  return out;
}

#endif  // DC_SAN_MAIN
