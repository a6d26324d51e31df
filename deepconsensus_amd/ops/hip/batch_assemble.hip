// batch_assemble / pool_store — device-side training input assembly.
//
// models/data_device.py keeps the shuffle pool in HBM and uploads raw
// tf.Example payloads; these two kernels do the per-element work of
// data.format_rows + train._prepare_batch (and the optional label left
// shift) on the way out of the pool. The packing, the host table validator
// and the numpy twins (batch_assemble_numpy, pool_store_numpy) live there.
//
//   pool   : fp32 [P, S]  shuffle pool, one example per slot
//   upload : fp32 [C, S]  this step's incoming examples; n_in <= C are live
//   slot   : R*L subread floats, zero-padded to a multiple of 4 floats,
//            then L label floats, padded likewise: S = pad4(R*L) + pad4(L)
//   gather : int32 [B]    g >= 0: pool slot g; g < 0: upload row ~g
//   scatter: int32 [n_in] pool slot that upload row i moves into, or -1
//
// batch_assemble, per output example b:
//   rows[b]  = the slot's R*L floats, with the PW, IP and SN row ranges
//              clipped to [0, max] (a max of 0 leaves the range alone, as
//              format_rows does). The ranges come in as element offsets
//              into the flat [R*L] row, so no lane divides.
//   label[b] = the slot's L label floats; with shift != 0 the non-gap
//              (!= 0) values move left in order and the gaps follow, also
//              in order (phred.left_shift_seq is that stable partition).
// pool_store moves upload row i into pool slot scatter[i]. When several
// rows name one slot the highest row wins: every workgroup looks for a
// later row with its destination and stands down if there is one, so the
// result does not depend on scheduling. It runs after batch_assemble of
// the same step on the same stream: the gather reads the old pool.
//
// Decomposition: one 256-thread workgroup per (example, 1/kSplit of the
// row). Consecutive lanes take consecutive float4s, so a wave load is one
// 1 KiB run; the slot stride is a multiple of 16 bytes, so every source
// float4 is aligned. The destination row b starts at b*R*L floats, which
// is 16-byte aligned for every b only when R*L % 4 == 0 and the tensor
// itself is: otherwise the same lanes store four dwords each. The R*L % 4
// tail goes scalar; nothing is read or written past a row. blockIdx.y == 0
// also owns the label. LDS is used by the label compaction only.
//
// Bounds: a gather entry is clamped into [0, P) or [0, n_in); an entry
// whose source set is empty yields zeros. A scatter entry outside [0, P)
// is skipped. The host validator rejects such tables before launch; the
// clamps make sure a bad table cannot become a wild access.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSplit = 4;  // workgroups per example row

struct ClipRanges {
  int pw_lo, pw_hi, ip_lo, ip_hi, sn_lo, sn_hi;  // element offsets in [R*L]
  float pw_max, ip_max, sn_max;                  // 0: leave alone
};

__device__ __forceinline__ float clip0(float x, float hi) {
  // np.clip order: max(x, 0) then min(.., hi); a NaN stays a NaN.
  x = x < 0.0f ? 0.0f : x;
  return x > hi ? hi : x;
}

__device__ __forceinline__ float clip_elem(float x, int e,
                                           const ClipRanges& c) {
  if (e >= c.pw_lo && e < c.pw_hi) return clip0(x, c.pw_max);
  if (e >= c.ip_lo && e < c.ip_hi) return clip0(x, c.ip_max);
  if (e >= c.sn_lo && e < c.sn_hi) return clip0(x, c.sn_max);
  return x;
}

template <bool kVecStore>
__global__ __launch_bounds__(kThreads) void batch_assemble_kernel(
    const float* __restrict__ pool, const float* __restrict__ upload,
    const int* __restrict__ gather, float* __restrict__ rows,
    float* __restrict__ label, int P, int n_in, int RL, int L, int S,
    int label_off, ClipRanges clip, int shift) {
  __shared__ int s_keep[kWaves];

  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int g = gather[b];
  const float* src = nullptr;
  if (g >= 0) {
    if (P > 0) src = pool + (size_t)(g < P ? g : P - 1) * S;
  } else {
    const int u = ~g;
    if (n_in > 0) src = upload + (size_t)(u < n_in ? u : n_in - 1) * S;
  }
  float* dst = rows + (size_t)b * RL;

  const int nv = RL >> 2;
  for (int v = blockIdx.y * kThreads + tid; v < nv; v += kSplit * kThreads) {
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    if (src) x = reinterpret_cast<const float4*>(src)[v];
    const int e = v << 2;
    // A float4 lies inside one clip range or outside all of them unless
    // it straddles a range end; the per-element test covers both.
    x.x = clip_elem(x.x, e, clip);
    x.y = clip_elem(x.y, e + 1, clip);
    x.z = clip_elem(x.z, e + 2, clip);
    x.w = clip_elem(x.w, e + 3, clip);
    if (kVecStore) {
      reinterpret_cast<float4*>(dst)[v] = x;
    } else {
      dst[e] = x.x;
      dst[e + 1] = x.y;
      dst[e + 2] = x.z;
      dst[e + 3] = x.w;
    }
  }
  if (blockIdx.y != 0) return;

  // Scalar tail of the row: RL % 4 floats.
  {
    const int e = (nv << 2) + tid;
    if (e < RL) dst[e] = clip_elem(src ? src[e] : 0.0f, e, clip);
  }

  // Label.
  const float* lsrc = src ? src + label_off : nullptr;
  float* ldst = label + (size_t)b * L;
  if (!shift) {
    for (int c = tid; c < L; c += kThreads) ldst[c] = lsrc ? lsrc[c] : 0.0f;
    return;
  }
  // Stable partition, kThreads columns per pass: kept values first. Pass 1
  // counts the kept values of the whole row, pass 2 places both classes.
  const int lane = tid & 63;
  const int wave = tid >> 6;
  int total = 0;
  for (int c0 = 0; c0 < L; c0 += kThreads) {
    const int c = c0 + tid;
    const float v = (c < L && lsrc) ? lsrc[c] : 0.0f;
    const bool keep = (c < L) && (v != 0.0f);
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) s_keep[wave] = __popcll(mask);
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kWaves; ++w) total += s_keep[w];
    __syncthreads();
  }
  int kept_before = 0;  // kept values in earlier passes
  for (int c0 = 0; c0 < L; c0 += kThreads) {
    const int c = c0 + tid;
    const bool in = c < L;
    const float v = (in && lsrc) ? lsrc[c] : 0.0f;
    const bool keep = in && (v != 0.0f);
    const unsigned long long mask = __ballot(keep);
    const int prefix = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) s_keep[wave] = __popcll(mask);
    __syncthreads();
    int wave_base = 0, pass_kept = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const int n = s_keep[w];
      if (w < wave) wave_base += n;
      pass_kept += n;
    }
    if (in) {
      const int kept_lt = kept_before + wave_base + prefix;  // kept before c
      const int pos = keep ? kept_lt : total + (c - kept_lt);
      ldst[pos] = v;  // pos < L: kept_lt <= c and total <= L - gaps
    }
    kept_before += pass_kept;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads) void pool_store_kernel(
    float* __restrict__ pool, const float* __restrict__ upload,
    const int* __restrict__ scatter, int P, int n_in, int S) {
  const int i = blockIdx.x;
  const int tid = threadIdx.x;
  const int d = scatter[i];
  if (d < 0 || d >= P) return;  // uniform per workgroup
  int later = 0;
  for (int k = i + 1 + tid; k < n_in; k += kThreads) later |= scatter[k] == d;
  if (__syncthreads_or(later)) return;
  const float4* src = reinterpret_cast<const float4*>(upload + (size_t)i * S);
  float4* dst = reinterpret_cast<float4*>(pool + (size_t)d * S);
  const int nv = S >> 2;  // S % 4 == 0
  for (int v = blockIdx.y * kThreads + tid; v < nv; v += kSplit * kThreads) {
    dst[v] = src[v];
  }
}

void check_slots(const at::Tensor& t, const char* name, int64_t S) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat &&
                  t.is_contiguous() && t.dim() == 2,
              name, " must be a contiguous fp32 [n, S] device tensor");
  TORCH_CHECK(t.size(1) == S, name, " has slot stride ", t.size(1),
              ", expected ", S);
  TORCH_CHECK(t.size(0) < (int64_t(1) << 31), name, " has too many slots");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name,
              " must be 16-byte aligned");
}

void check_table(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kInt &&
                  t.is_contiguous() && t.dim() == 1,
              name, " must be a contiguous int32 1-D device tensor");
}

int64_t pad4(int64_t n) { return (n + 3) & ~int64_t(3); }

}  // namespace

int64_t batch_assemble_slot_floats(int64_t R, int64_t L) {
  return pad4(R * L) + pad4(L);
}

void batch_assemble_into(at::Tensor pool, at::Tensor upload, int64_t n_in,
                         at::Tensor gather, at::Tensor rows, at::Tensor label,
                         int64_t max_passes, bool use_ccs_bq, double pw_max,
                         double ip_max, double sn_max,
                         bool remove_label_gaps) {
  TORCH_CHECK(rows.is_cuda() && rows.scalar_type() == at::kFloat &&
                  rows.is_contiguous() && rows.dim() == 3,
              "rows must be a contiguous fp32 [B, R, L] device tensor");
  const int64_t B = rows.size(0), R = rows.size(1), L = rows.size(2);
  TORCH_CHECK(R >= 1 && L >= 1 && R * L < (int64_t(1) << 30),
              "rows has an unsupported shape");
  TORCH_CHECK(label.is_cuda() && label.scalar_type() == at::kFloat &&
                  label.is_contiguous() && label.dim() == 2 &&
                  label.size(0) == B && label.size(1) == L,
              "label must be a contiguous fp32 [B, L] device tensor");
  const int64_t S = batch_assemble_slot_floats(R, L);
  check_slots(pool, "pool", S);
  check_slots(upload, "upload", S);
  check_table(gather, "gather");
  TORCH_CHECK(gather.numel() == B, "gather must have one entry per example");
  TORCH_CHECK(n_in >= 0 && n_in <= upload.size(0),
              "n_in must lie in [0, upload rows]");
  TORCH_CHECK(pool.device() == rows.device() &&
                  upload.device() == rows.device() &&
                  gather.device() == rows.device() &&
                  label.device() == rows.device(),
              "all tensors must be on the same device");
  const int64_t sn0 = 4 * max_passes + 1 + (use_ccs_bq ? 1 : 0);
  TORCH_CHECK(max_passes >= 0 && sn0 + 4 <= R,
              "max_passes / use_ccs_bq do not fit ", R, " rows");
  if (B == 0) return;
  TORCH_CHECK(B < (int64_t(1) << 31), "too many examples");

  ClipRanges c;
  c.pw_max = (float)pw_max;
  c.ip_max = (float)ip_max;
  c.sn_max = (float)sn_max;
  // An empty range switches its clip off.
  c.pw_lo = (int)(max_passes * L);
  c.pw_hi = pw_max != 0 ? (int)(2 * max_passes * L) : c.pw_lo;
  c.ip_lo = (int)(2 * max_passes * L);
  c.ip_hi = ip_max != 0 ? (int)(3 * max_passes * L) : c.ip_lo;
  c.sn_lo = (int)(sn0 * L);
  c.sn_hi = sn_max != 0 ? (int)((sn0 + 4) * L) : c.sn_lo;

  const bool vec = (R * L) % 4 == 0 &&
                   reinterpret_cast<uintptr_t>(rows.data_ptr()) % 16 == 0;
  const dim3 grid((unsigned)B, kSplit);
  hipStream_t stream = at::hip::getCurrentHIPStream();
  auto launch = vec ? batch_assemble_kernel<true>
                    : batch_assemble_kernel<false>;
  hipLaunchKernelGGL(launch, grid, dim3(kThreads), 0, stream,
                     pool.data_ptr<float>(), upload.data_ptr<float>(),
                     gather.data_ptr<int>(), rows.data_ptr<float>(),
                     label.data_ptr<float>(), (int)pool.size(0), (int)n_in,
                     (int)(R * L), (int)L, (int)S, (int)pad4(R * L), c,
                     remove_label_gaps ? 1 : 0);
}

void pool_store(at::Tensor pool, at::Tensor upload, at::Tensor scatter) {
  TORCH_CHECK(pool.dim() == 2, "pool must be [P, S]");
  const int64_t S = pool.size(1);
  TORCH_CHECK(S % 4 == 0, "slot stride must be a multiple of 4 floats");
  check_slots(pool, "pool", S);
  check_slots(upload, "upload", S);
  check_table(scatter, "scatter");
  const int64_t n_in = scatter.numel();
  TORCH_CHECK(n_in <= upload.size(0),
              "scatter has more entries than upload has rows");
  TORCH_CHECK(upload.device() == pool.device() &&
                  scatter.device() == pool.device(),
              "all tensors must be on the same device");
  if (n_in == 0 || pool.size(0) == 0) return;
  hipStream_t stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(pool_store_kernel, dim3((unsigned)n_in, kSplit),
                     dim3(kThreads), 0, stream, pool.data_ptr<float>(),
                     upload.data_ptr<float>(), scatter.data_ptr<int>(),
                     (int)pool.size(0), (int)n_in, (int)S);
}
