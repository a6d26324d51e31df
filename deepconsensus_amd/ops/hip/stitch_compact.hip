// stitch_compact — device-side window stitching (gap compaction).
//
// The model emits one base id (0 = gap, 1..4 = ATCG) and one Phred QV per
// window position. Stitching a read concatenates its windows and drops the
// gap positions together with their QVs (postprocess/stitch.py:
// get_full_sequence + remove_gaps). That is a segmented stream compaction:
//
//   bases, quals : flat uint8 source buffers of equal length
//   seg_off[S], seg_len[S] : source byte range of each segment, listed in
//                            OUTPUT order (any offset, any length, 0 allowed)
//   seg_kept[S]  : non-gap count per segment
//   out_off[S+1] : exclusive prefix sum of seg_kept
//   seq_out[out_off[S]]  : kept ids as ASCII through SEQ_VOCAB (" ATCG")
//   qual_out[out_off[S]] : kept QVs + 33
//
// Two passes, one wave64 per segment, no atomics:
//   stitch_count   — lanes stride the segment; __ballot + popcount.
//   (exclusive scan of the counts: torch cumsum in the wrapper)
//   stitch_scatter — same traversal; a kept lane writes at
//                    out_off[s] + running + popcount(ballot below its lane).
//
// Byte loads and byte stores only: passthrough segments sit at arbitrary
// offsets and the packed destination is unaligned by construction. A wave
// reads 64 consecutive bytes per step, which is one fully used 64 B
// request; the whole job moves a few MB per ZMW batch and is launch-bound.
//
// Bounds: a segment is clamped to the source buffer ([0, n_src)) in both
// passes identically, so a malformed table can neither read outside
// `bases`/`quals` nor desynchronise count and scatter; the scatter also
// refuses any destination >= n_out.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

namespace {

constexpr int kWavesPerBlock = 4;
constexpr int kMaxBlocks = 4096;
// SEQ_VOCAB " ATCG" packed little-endian: byte k is the ASCII of id k.
constexpr unsigned long long kVocabPacked = 0x4743544120ull;

// Clamps (off, len) to [0, n_src); returns the usable length.
__device__ __forceinline__ int clamp_segment(int off, int len, int n_src) {
  if (off < 0 || off >= n_src || len <= 0) return 0;
  const int room = n_src - off;
  return len < room ? len : room;
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void stitch_count_kernel(
    const uint8_t* __restrict__ bases, const int* __restrict__ seg_off,
    const int* __restrict__ seg_len, int* __restrict__ seg_kept, int S,
    int n_src) {
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  for (int s = blockIdx.x * kWavesPerBlock + wave; s < S;
       s += gridDim.x * kWavesPerBlock) {
    const int off = seg_off[s];
    const int len = clamp_segment(off, seg_len[s], n_src);
    const uint8_t* src = bases + off;
    int kept = 0;
    // `start` and `len` are wave-uniform: every lane runs every step, so
    // the ballot always sees the whole wave.
    for (int start = 0; start < len; start += 64) {
      const int i = start + lane;
      const bool keep = i < len && src[i] != 0;
      kept += __popcll(__ballot(keep));
    }
    if (lane == 0) seg_kept[s] = kept;
  }
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void stitch_scatter_kernel(
    const uint8_t* __restrict__ bases, const uint8_t* __restrict__ quals,
    const int* __restrict__ seg_off, const int* __restrict__ seg_len,
    const int* __restrict__ out_off, uint8_t* __restrict__ seq_out,
    uint8_t* __restrict__ qual_out, int S, int n_src, int n_out) {
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int s = blockIdx.x * kWavesPerBlock + wave; s < S;
       s += gridDim.x * kWavesPerBlock) {
    const int off = seg_off[s];
    const int len = clamp_segment(off, seg_len[s], n_src);
    const uint8_t* src_b = bases + off;
    const uint8_t* src_q = quals + off;
    int running = out_off[s];
    for (int start = 0; start < len; start += 64) {
      const int i = start + lane;
      uint8_t b = 0, q = 0;
      if (i < len) {
        b = src_b[i];
        q = src_q[i];
      }
      const bool keep = b != 0;
      const unsigned long long mask = __ballot(keep);
      const int dst = running + __popcll(mask & below);
      if (keep && dst < n_out) {
        // Ids above 4 are outside the vocabulary; they surface as 'N'.
        seq_out[dst] =
            b < 5 ? (uint8_t)((kVocabPacked >> (8 * b)) & 0xffull)
                  : (uint8_t)'N';
        qual_out[dst] = (uint8_t)(q + 33);
      }
      running += __popcll(mask);
    }
  }
}

void check_u8(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a device tensor");
  TORCH_CHECK(t.scalar_type() == at::kByte, name, " must be uint8");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.dim() == 1, name, " must be 1-D");
}

void check_i32(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a device tensor");
  TORCH_CHECK(t.scalar_type() == at::kInt, name, " must be int32");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.dim() == 1, name, " must be 1-D");
}

void check_inputs(const at::Tensor& bases, const at::Tensor& quals,
                  const at::Tensor& seg_off, const at::Tensor& seg_len) {
  check_u8(bases, "bases");
  check_u8(quals, "quals");
  check_i32(seg_off, "seg_off");
  check_i32(seg_len, "seg_len");
  TORCH_CHECK(bases.numel() == quals.numel(),
              "bases and quals must have equal length");
  TORCH_CHECK(bases.numel() < (int64_t(1) << 31),
              "source buffer must be shorter than 2^31 bytes");
  TORCH_CHECK(seg_off.numel() == seg_len.numel(),
              "seg_off and seg_len must have equal length");
  TORCH_CHECK(seg_off.numel() < (int64_t(1) << 31) - 1,
              "too many segments");
  TORCH_CHECK(quals.device() == bases.device() &&
                  seg_off.device() == bases.device() &&
                  seg_len.device() == bases.device(),
              "all tensors must be on the same device");
}

dim3 grid_for(int S) {
  const int blocks = (S + kWavesPerBlock - 1) / kWavesPerBlock;
  return dim3(std::max(1, std::min(blocks, kMaxBlocks)));
}

// Pass 1 + scan. Fills seg_kept[S] and out_off[S+1]; returns out_off[S]
// (one scalar D2H, which the caller needs to size the output anyway).
int64_t count_and_scan(const at::Tensor& bases, const at::Tensor& seg_off,
                       const at::Tensor& seg_len, at::Tensor& seg_kept,
                       at::Tensor& out_off, hipStream_t stream) {
  const int S = (int)seg_off.numel();
  out_off.zero_();
  if (S == 0) return 0;
  hipLaunchKernelGGL(stitch_count_kernel, grid_for(S),
                     dim3(64 * kWavesPerBlock), 0, stream,
                     bases.data_ptr<uint8_t>(), seg_off.data_ptr<int>(),
                     seg_len.data_ptr<int>(), seg_kept.data_ptr<int>(), S,
                     (int)bases.numel());
  // Scan in int64: overlapping segments may total more than the source.
  auto scan = at::cumsum(seg_kept, 0, at::kLong);
  const int64_t total = scan[S - 1].item<int64_t>();
  TORCH_CHECK(total < (int64_t(1) << 31),
              "compacted output must be shorter than 2^31 bytes");
  out_off.narrow(0, 1, S).copy_(scan);
  return total;
}

void scatter(const at::Tensor& bases, const at::Tensor& quals,
             const at::Tensor& seg_off, const at::Tensor& seg_len,
             const at::Tensor& out_off, at::Tensor& seq_out,
             at::Tensor& qual_out, int64_t total, hipStream_t stream) {
  const int S = (int)seg_off.numel();
  if (S == 0 || total == 0) return;
  hipLaunchKernelGGL(stitch_scatter_kernel, grid_for(S),
                     dim3(64 * kWavesPerBlock), 0, stream,
                     bases.data_ptr<uint8_t>(), quals.data_ptr<uint8_t>(),
                     seg_off.data_ptr<int>(), seg_len.data_ptr<int>(),
                     out_off.data_ptr<int>(), seq_out.data_ptr<uint8_t>(),
                     qual_out.data_ptr<uint8_t>(), S, (int)bases.numel(),
                     (int)total);
}

}  // namespace

std::vector<at::Tensor> stitch_compact(at::Tensor bases, at::Tensor quals,
                                       at::Tensor seg_off,
                                       at::Tensor seg_len) {
  check_inputs(bases, quals, seg_off, seg_len);
  const int64_t S = seg_off.numel();
  auto iopts = seg_off.options();
  auto seg_kept = at::empty({S}, iopts);
  auto out_off = at::empty({S + 1}, iopts);
  hipStream_t stream = at::hip::getCurrentHIPStream();
  const int64_t total =
      count_and_scan(bases, seg_off, seg_len, seg_kept, out_off, stream);
  auto seq_out = at::empty({total}, bases.options());
  auto qual_out = at::empty({total}, bases.options());
  scatter(bases, quals, seg_off, seg_len, out_off, seq_out, qual_out, total,
          stream);
  return {seq_out, qual_out, seg_kept, out_off};
}

// Same computation into caller-owned buffers (possibly views of larger
// allocations). seq_out/qual_out must hold at least out_off[S] bytes;
// nothing past out_off[S] is written. Returns out_off[S].
int64_t stitch_compact_into(at::Tensor bases, at::Tensor quals,
                            at::Tensor seg_off, at::Tensor seg_len,
                            at::Tensor seq_out, at::Tensor qual_out,
                            at::Tensor seg_kept, at::Tensor out_off) {
  check_inputs(bases, quals, seg_off, seg_len);
  check_u8(seq_out, "seq_out");
  check_u8(qual_out, "qual_out");
  check_i32(seg_kept, "seg_kept");
  check_i32(out_off, "out_off");
  const int64_t S = seg_off.numel();
  TORCH_CHECK(seg_kept.numel() == S, "seg_kept must have S elements");
  TORCH_CHECK(out_off.numel() == S + 1, "out_off must have S+1 elements");
  TORCH_CHECK(seq_out.device() == bases.device() &&
                  qual_out.device() == bases.device() &&
                  seg_kept.device() == bases.device() &&
                  out_off.device() == bases.device(),
              "all tensors must be on the same device");
  hipStream_t stream = at::hip::getCurrentHIPStream();
  const int64_t total =
      count_and_scan(bases, seg_off, seg_len, seg_kept, out_off, stream);
  TORCH_CHECK(seq_out.numel() >= total && qual_out.numel() >= total,
              "output buffers hold fewer than out_off[S] = ", total,
              " bytes");
  scatter(bases, quals, seg_off, seg_len, out_off, seq_out, qual_out, total,
          stream);
  return total;
}
