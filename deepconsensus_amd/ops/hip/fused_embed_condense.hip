// Embedding gather fused into the condenser for gfx950 (K2 + K3 + K4):
//   out = concat_r(table_r[id_r]) @ W^T + pos
//
// fused_condense reads each 16-byte A fragment of the concatenated
// embedding [M, K] exactly once, and embed_gather wrote that tensor only to
// be read back: 2 x 1.83 GB of HBM traffic at M = 1.6 M rows for data that
// is a function of 85 int16 ids per position and ~16 KB of tables. Here the
// condenser's prologue fetches every fragment from the tables instead. The
// tile core (weight stream, MFMA chunk loop, epilogue) is condense_tile.h,
// shared with fused_condense; the output is bit-for-bit
//   fused_condense(embed_gather(rows, ...).reshape(B*L, K), w, pos, n, L).
//
// One A fragment is one 16-byte chunk of embed_gather's host-built map:
// lane (c, hi), granule s, holds chunk 2*s + hi of row m0 + 32*wave + c.
// A chunk is one width-8 table row, or up to four width-2 entries that
// each fill one dword (runner.build_gather_tables).
//
// The chunk index depends on the lane only through hi, so the map entry,
// the row's id shift and its vocabulary are wave-uniform pairs: they are
// read with constant / scalar-register indices (scalar loads), selected by
// hi, and only the id and the table row are per-lane vector loads. That is
// the fast path, taken when both chunks of a granule are single width-8
// entries (65 of 70 chunks at K = 560). A granule with a width-2 chunk in
// either half takes the per-lane path, which is embed_gather's code: four
// statically indexed u32 loads under k < cnt, no runtime-depth loop and no
// 64-bit shift accumulation (profiles/r02_embed_gather_bug.md).
//
// Id loads: lanes 0-31 / 32-63 each read 32 consecutive positions of one
// input row (64 contiguous bytes at int16), split only where the 32-row
// group crosses a window boundary. Tables and map stay in global memory
// (L1/L2 resident). Rows >= M issue no loads and hold zero fragments.

#ifndef DC_SAN_MAIN
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#endif
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include "condense_tile.h"

namespace {

constexpr int MAX_R = 160;   // input rows supported, as embed_gather

// id of the input row at element offset off = r * L from this lane's
// position in row 0 of its window: the same conversion, shift
// and clamp as embed_gather (which narrows the clamped id to int16).
template <typename TIn>
__device__ __forceinline__ int cond_row_id(const TIn* __restrict__ rp,
                                           size_t off, int shift,
                                           int vocab) {
  const int id = (int)rp[off] + shift;
  const int vmax = vocab - 1;
  return (short)(id < 0 ? 0 : (id > vmax ? vmax : id));
}

// One 16-byte chunk, per-lane map lookups: embed_gather's body.
template <typename TIn>
__device__ __forceinline__ bf16x8 cond_gather_chunk(
    const TIn* __restrict__ rp, const bf16* __restrict__ table_flat,
    const int* __restrict__ row_shift, const int* __restrict__ row_vocab,
    const int4* __restrict__ chunk_entries, int c, int cnt, int L) {
  uint4 raw;
  if (cnt == 1) {
    const int4 e = chunk_entries[c * 4];
    const int id = cond_row_id(rp, (size_t)e.x * L, row_shift[e.x],
                               row_vocab[e.x]);
    raw = *reinterpret_cast<const uint4*>(table_flat + e.y + (size_t)id * 8);
  } else {
    unsigned d[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < cnt) {
        const int4 e = chunk_entries[c * 4 + k];
        const int id = cond_row_id(rp, (size_t)e.x * L, row_shift[e.x],
                                   row_vocab[e.x]);
        d[k] = *reinterpret_cast<const unsigned*>(
            table_flat + e.y + (size_t)id * 2);
      }
    }
    raw.x = d[0];
    raw.y = d[1];
    raw.z = d[2];
    raw.w = d[3];
  }
  return __builtin_bit_cast(bf16x8, raw);
}

template <int K, typename TIn>
__global__ __launch_bounds__(CondCfg<K>::NT, 1)
void fused_embed_condense_kernel(
    const TIn* __restrict__ rows,            // [B, R, L]
    const bf16* __restrict__ table_flat,     // concatenated scaled tables
    const int* __restrict__ row_shift,       // [R]
    const int* __restrict__ row_vocab,       // [R]
    const int* __restrict__ chunk_cnt,       // [K / 8]
    const int4* __restrict__ chunk_entries,  // [K / 8 * 4] (row, base, w, -)
    const bf16* __restrict__ w, const float* __restrict__ pos,
    bf16* __restrict__ out, int M, int N, int Npad, int R, int L) {
  using C = CondCfg<K>;
  constexpr int NG = C::NG;
  constexpr int BM = C::BM;
  __shared__ __attribute__((aligned(16))) bf16 w_lds[NC * C::WS];
  __shared__ __attribute__((aligned(16))) bf16 o_lds[BM * O_STRIDE];

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0 = blockIdx.x * BM;

  cond_issue_w<K>(w, w_lds, wave, 0);

  bf16x8 af[NG];
  {
    const int ln = lane_recompute();
    const int row = m0 + 32 * wave + (ln & 31);
    const int hi = ln >> 5;
    // Granules whose two chunks (2s, 2s+1) both exist.
    constexpr int NFULL = C::HALF ? NG - 1 : NG;
    if (row < M) {
      const int b = row / L;
      const TIn* rp = rows + (size_t)b * R * L + (row - b * L);
#pragma unroll
      for (int s = 0; s < NFULL; ++s) {
        const int cnt0 = chunk_cnt[2 * s], cnt1 = chunk_cnt[2 * s + 1];
        if (cnt0 == 1 && cnt1 == 1) {
          // Both halves are one width-8 entry: map, shift and vocab by
          // scalar loads, selected by hi.
          const int4 e0 = chunk_entries[8 * s];
          const int4 e1 = chunk_entries[8 * s + 4];
          const int sh0 = row_shift[e0.x], sh1 = row_shift[e1.x];
          const int vc0 = row_vocab[e0.x], vc1 = row_vocab[e1.x];
          const size_t o0 = (size_t)e0.x * L, o1 = (size_t)e1.x * L;
          const int id = cond_row_id(rp, hi ? o1 : o0, hi ? sh1 : sh0,
                                     hi ? vc1 : vc0);
          af[s] = *reinterpret_cast<const bf16x8*>(
              table_flat + (hi ? e1.y : e0.y) + (size_t)id * 8);
        } else {
          af[s] = cond_gather_chunk(rp, table_flat, row_shift, row_vocab,
                                    chunk_entries, 2 * s + hi,
                                    hi ? cnt1 : cnt0, L);
        }
      }
      if constexpr (C::HALF) {
        // Chunk 2*(NG-1) belongs to the hi = 0 lanes; chunk 2*(NG-1)+1
        // does not exist: zero, and nothing is looked up for it.
        af[NG - 1] = bf16x8{};
        if (hi == 0) {
          af[NG - 1] = cond_gather_chunk(
              rp, table_flat, row_shift, row_vocab, chunk_entries,
              2 * (NG - 1), chunk_cnt[2 * (NG - 1)], L);
        }
      }
    } else {
#pragma unroll
      for (int s = 0; s < NG; ++s) af[s] = bf16x8{};
    }
  }
  cond_chunk_loop<K>(af, w, pos, out, w_lds, o_lds, M, N, Npad, L, tid, wave,
                     m0);
}

// Explicit instantiations: the four served widths x the two id types.
#define DC_EMBED_CONDENSE_INST(K, T)                                       \
  template __global__ void fused_embed_condense_kernel<K, T>(              \
      const T* __restrict__, const bf16* __restrict__,                     \
      const int* __restrict__, const int* __restrict__,                    \
      const int* __restrict__, const int4* __restrict__,                   \
      const bf16* __restrict__, const float* __restrict__,                 \
      bf16* __restrict__, int, int, int, int, int)
DC_EMBED_CONDENSE_INST(560, short);
DC_EMBED_CONDENSE_INST(568, short);
DC_EMBED_CONDENSE_INST(872, short);
DC_EMBED_CONDENSE_INST(880, short);
DC_EMBED_CONDENSE_INST(560, float);
DC_EMBED_CONDENSE_INST(568, float);
DC_EMBED_CONDENSE_INST(872, float);
DC_EMBED_CONDENSE_INST(880, float);
#undef DC_EMBED_CONDENSE_INST

}  // namespace

#ifndef DC_SAN_MAIN

namespace {

template <int K, typename TIn>
void launch_embed_condense(const at::Tensor& rc, const at::Tensor& table_flat,
                           const at::Tensor& row_shift,
                           const at::Tensor& row_vocab,
                           const at::Tensor& chunk_cnt,
                           const at::Tensor& chunk_entries,
                           const at::Tensor& w, const float* pos_ptr,
                           at::Tensor& out, int M, int N, int Npad, int R,
                           int L) {
  using C = CondCfg<K>;
  TORCH_CHECK(w.size(1) == C::WS, "fused_embed_condense: width-", K,
              " input needs a weight image of row stride ", C::WS,
              ", got ", w.size(1));
  dim3 grid((M + C::BM - 1) / C::BM);
  dim3 block(C::NT);
  hipStream_t stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL((fused_embed_condense_kernel<K, TIn>), grid, block, 0,
                     stream, rc.data_ptr<TIn>(),
                     reinterpret_cast<bf16*>(table_flat.data_ptr()),
                     row_shift.data_ptr<int>(), row_vocab.data_ptr<int>(),
                     chunk_cnt.data_ptr<int>(),
                     reinterpret_cast<int4*>(chunk_entries.data_ptr<int>()),
                     reinterpret_cast<bf16*>(w.data_ptr()), pos_ptr,
                     reinterpret_cast<bf16*>(out.data_ptr()), M, N, Npad, R,
                     L);
}

template <typename TIn, typename... Args>
void dispatch_embed_condense(int K, Args&&... args) {
  switch (K) {
    case 560: launch_embed_condense<560, TIn>(args...); break;
    case 568: launch_embed_condense<568, TIn>(args...); break;
    case 872: launch_embed_condense<872, TIn>(args...); break;
    default:  launch_embed_condense<880, TIn>(args...); break;
  }
}

}  // namespace

at::Tensor fused_embed_condense(
    at::Tensor rows, at::Tensor table_flat, at::Tensor row_shift,
    at::Tensor row_vocab, at::Tensor chunk_cnt, at::Tensor chunk_entries,
    at::Tensor w, at::Tensor pos, int64_t n_out) {
  TORCH_CHECK(rows.is_cuda() && rows.dim() == 3 &&
                  (rows.dtype() == at::kFloat || rows.dtype() == at::kShort),
              "rows must be float32 or int16 [B, R, L] on device");
  TORCH_CHECK(table_flat.is_cuda() && table_flat.is_contiguous() &&
                  table_flat.dtype() == at::kBFloat16,
              "tables must be contiguous bf16 on device");
  auto rc = rows.contiguous();
  const int B = rc.size(0), R = rc.size(1), L = rc.size(2);
  TORCH_CHECK(R <= MAX_R, "too many rows");
  auto is_map = [](const at::Tensor& t) {
    return t.is_cuda() && t.is_contiguous() && t.dtype() == at::kInt;
  };
  TORCH_CHECK(is_map(row_shift) && is_map(row_vocab) && is_map(chunk_cnt) &&
                  is_map(chunk_entries),
              "gather map tensors must be contiguous int32 on device");
  TORCH_CHECK(row_shift.numel() == R && row_vocab.numel() == R,
              "row_shift / row_vocab must have one entry per input row (", R,
              ")");
  const int nchunk = chunk_cnt.numel();
  const int K = 8 * nchunk;
  TORCH_CHECK(K == 560 || K == 568 || K == 872 || K == 880,
              "fused_embed_condense requires concat width 560, 568, 872 or "
              "880, got ", K);
  TORCH_CHECK(chunk_entries.numel() == (int64_t)nchunk * 16,
              "chunk_entries must hold 4 x int4 per chunk");
  TORCH_CHECK(w.is_cuda() && w.dim() == 2 && w.is_contiguous() &&
                  w.dtype() == at::kBFloat16 && w.size(0) % NC == 0,
              "w must be contiguous bf16 [Npad (mult of 64), WS] on device");
  const int Npad = w.size(0);
  const int N = (int)n_out;
  TORCH_CHECK(N <= Npad, "n_out exceeds padded weight rows");
  const int64_t M64 = (int64_t)B * L;
  TORCH_CHECK(M64 < (1LL << 31) - 256, "too many positions");
  const int M = (int)M64;
  const float* pos_ptr = nullptr;
  at::Tensor pc;
  if (pos.defined() && pos.numel() > 0) {
    pc = pos.contiguous();
    TORCH_CHECK(pc.is_cuda() && pc.dtype() == at::kFloat &&
                    pc.size(-1) == N && pc.numel() >= (int64_t)L * N,
                "pos must be fp32 [>=L, N] on device");
    pos_ptr = pc.data_ptr<float>();
  }
  auto out = at::empty({M, N}, rc.options().dtype(at::kBFloat16));
  if (M == 0) return out;
  if (rc.dtype() == at::kFloat) {
    dispatch_embed_condense<float>(K, rc, table_flat, row_shift, row_vocab,
                                   chunk_cnt, chunk_entries, w, pos_ptr, out,
                                   M, N, Npad, R, L);
  } else {
    dispatch_embed_condense<short>(K, rc, table_flat, row_shift, row_vocab,
                                   chunk_cnt, chunk_entries, w, pos_ptr, out,
                                   M, N, Npad, R, L);
  }
  return out;
}

#endif  // DC_SAN_MAIN
