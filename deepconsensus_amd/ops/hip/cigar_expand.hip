// cigar_expand — device-side alignment expansion of raw BAM records.
//
// Writes the unspaced element stream of every read, codes[n] | pw[n] | ip[n],
// into the src buffer that subread_space reads, from the record's own
// operands (4-bit packed sequence, pw and ip tag arrays) and a normalized op
// table. preprocess/expand_device.py holds the worker side, the packing, the
// host validator and the numpy twin (expand_reads_numpy); expand.py and the
// C++ expand_read are the semantics.
//
// Inputs (all caller-owned):
//   raw    : uint8. Per read packed_seq[(l_seq + 1) / 2] | pw[l_seq] |
//            ip[l_seq]; base q of the sequence is the high half of byte
//            q >> 1 for even q, the low half for odd q.
//   op_tab : int32 [n, 3] = kind, out_start, q_start. Kinds: 0 EMIT, 1
//            EMIT_INS (code bit 0x80), 2 GAP, 3 DROP (no output), 4 END (the
//            sentinel row out_start = n_elem, q_start = l_seq). out_start /
//            q_start are exclusive prefix sums of the elements emitted / the
//            query consumed.
//   xr_tab : int64 [Rn, 8] = dst_off (in src), n_elem, op0, n_ops (sentinel
//            included), seq_off, l_seq, tag_off (pw; ip at tag_off + l_seq),
//            reverse.
//   lut    : 16 base ids by 4-bit code, passed by value.
// Output: src (uint8), 3 * n_elem bytes per read at dst_off.
//
// Element e belongs to the last row with out_start <= e, so rows without
// output are never selected. With q = q_start + (e - out_start) an EMIT row
// gives (lut[nibble q], pw[t], ip[t]), t = q forward and l_seq - 1 - q
// reverse; EMIT_INS the same with 0x80 on the code; anything else (0, 0, 0).
//
// One workgroup per read, walking the read in tiles of kTile elements, each
// lane kPerLane of them at a stride of kThreads, so the lanes of a wave store
// consecutive bytes of each of the three streams. Per tile one binary search
// on out_start in global memory (the same in every lane) finds the row of the
// tile's end, which is also the first row of the next tile; the rows that
// cover the tile are staged in LDS, kStage rows at a time and one row
// beyond as the upper bound, and every lane binary-searches the staged
// out_start for its elements. A tile covered by more than kStage rows (short
// ops, rows without output) takes more than one stage; an element is written
// in the stage that holds its row.
//
// Bounds: nothing is trusted. A read whose op rows, operands or destination
// do not lie inside op_tab / raw / src is skipped whole; row indices are
// clamped to the read's rows, every search runs over at most n_ops rows, q
// is clamped to [0, l_seq) and t with it. With a valid table (the host
// validator) no clamp acts.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

namespace {

constexpr int kThreads = 256;
constexpr int kPerLane = 4;
constexpr int kTile = kThreads * kPerLane;
constexpr int kStage = 256;  // op rows per LDS stage
constexpr int kOpCols = 3;
constexpr int kXrCols = 8;
constexpr int kEmit = 0, kEmitIns = 1;

struct Lut {
  unsigned long long lo, hi;  // base ids of codes 0..7 and 8..15
};

struct ExpandSizes {
  long long n_raw, n_rows, n_src;
  int Rn;
};

// Last row i in [lo0, n) with out_start <= e, or lo0 when there is none;
// ``row`` returns out_start of row i. At most 32 steps.
template <typename F>
__device__ __forceinline__ long long last_row_at_or_before(F row,
                                                           long long lo0,
                                                           long long n,
                                                           long long e) {
  long long lo = lo0, hi = n;  // first row with out_start > e
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if ((long long)row(mid) <= e) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  return lo > lo0 ? lo - 1 : lo0;
}

__global__ __launch_bounds__(kThreads) void cigar_expand_kernel(
    const uint8_t* __restrict__ raw, const int* __restrict__ op_tab,
    const long long* __restrict__ xr_tab, uint8_t* __restrict__ src, Lut lut,
    ExpandSizes sz) {
  __shared__ int s_kind[kStage], s_out[kStage + 1], s_q[kStage];
  const long long r = blockIdx.x;
  if (r >= sz.Rn) return;
  const long long* x = xr_tab + r * kXrCols;
  const long long dst = x[0], n = x[1], op0 = x[2], n_ops = x[3];
  const long long seq_off = x[4], l_seq = x[5], tag_off = x[6];
  const bool reverse = x[7] != 0;
  // Uniform, as every check below. Sizes are < 2^31: no sum overflows.
  if (n < 0 || dst < 0 || dst > sz.n_src || n > (sz.n_src - dst) / 3) return;
  if (n_ops < 1 || op0 < 0 || op0 > sz.n_rows || n_ops > sz.n_rows - op0) {
    return;
  }
  if (l_seq < 0 || l_seq >= (1LL << 31) || seq_off < 0 ||
      seq_off > sz.n_raw || (l_seq + 1) / 2 > sz.n_raw - seq_off ||
      tag_off < 0 || tag_off > sz.n_raw ||
      l_seq > (sz.n_raw - tag_off) / 2) {
    return;
  }
  const int* rows = op_tab + op0 * kOpCols;
  const uint8_t* seq = raw + seq_off;
  const uint8_t* pw = raw + tag_off;
  const uint8_t* ip = pw + l_seq;
  auto global_out = [&](long long i) { return rows[i * kOpCols + 1]; };

  long long first = last_row_at_or_before(global_out, 0, n_ops, 0);
  for (long long base = 0; base < n; base += kTile) {
    const long long end = base + kTile < n ? base + kTile : n;
    // The row of element ``end``: the first row of the next tile, and no
    // earlier than the last row of this one.
    const long long last =
        last_row_at_or_before(global_out, first, n_ops, end);
    for (long long s0 = first; s0 <= last; s0 += kStage) {
      const int cnt = (int)(last + 1 - s0 < kStage ? last + 1 - s0 : kStage);
      __syncthreads();  // the previous stage has been read
      for (int i = threadIdx.x; i <= cnt; i += kThreads) {
        // Row s0 + cnt is the bound; past the read's rows it is "no bound".
        const long long g = s0 + i;
        const bool in = g < n_ops;
        const int out = in ? rows[g * kOpCols + 1] : 0x7fffffff;
        s_out[i] = out;
        if (i < cnt) {
          s_kind[i] = in ? rows[g * kOpCols] : -1;
          s_q[i] = in ? rows[g * kOpCols + 2] : 0;
        }
      }
      __syncthreads();
      const long long lo = s_out[0], bound = s_out[cnt];
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) {
        const long long e = base + k * kThreads + threadIdx.x;
        // The first stage also takes what lies before its first row.
        if (e >= end || e >= bound || (e < lo && s0 != first)) continue;
        const int j = (int)last_row_at_or_before(
            [&](long long i) { return s_out[i]; }, 0, cnt, e);
        const int kind = s_kind[j];
        uint8_t code = 0, pv = 0, iv = 0;
        if ((kind == kEmit || kind == kEmitIns) && l_seq > 0) {
          long long q = (long long)s_q[j] + (e - (long long)s_out[j]);
          q = q < 0 ? 0 : (q > l_seq - 1 ? l_seq - 1 : q);
          const long long t = reverse ? l_seq - 1 - q : q;
          const uint8_t byte = seq[q >> 1];
          const int nibble = (q & 1) ? (byte & 0xf) : (byte >> 4);
          const unsigned long long word = nibble < 8 ? lut.lo : lut.hi;
          code = (uint8_t)(word >> (8 * (nibble & 7)));
          if (kind == kEmitIns) code |= 0x80;
          pv = pw[t];
          iv = ip[t];
        }
        src[dst + e] = code;
        src[dst + n + e] = pv;
        src[dst + 2 * n + e] = iv;
      }
    }
    first = last;
  }
}

void check_dev(const at::Tensor& t, at::ScalarType type, const char* name,
               const at::Tensor& like) {
  TORCH_CHECK(t.is_cuda(), name, " must be a device tensor");
  TORCH_CHECK(t.scalar_type() == type, name, " must be ", type);
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.numel() < (int64_t(1) << 31), name,
              " must be shorter than 2^31 elements");
  TORCH_CHECK(t.device() == like.device(),
              "all tensors must be on the same device");
}

}  // namespace

int64_t cigar_expand_tile() { return kTile; }

int64_t cigar_expand_stage() { return kStage; }

void cigar_expand_into(at::Tensor raw, at::Tensor op_tab, at::Tensor xr_tab,
                       at::Tensor src, at::Tensor lut) {
  check_dev(raw, at::kByte, "raw", raw);
  check_dev(op_tab, at::kInt, "op_tab", raw);
  check_dev(xr_tab, at::kLong, "xr_tab", raw);
  check_dev(src, at::kByte, "src", raw);
  TORCH_CHECK(raw.dim() == 1 && src.dim() == 1, "raw and src must be 1-D");
  TORCH_CHECK(op_tab.dim() == 2 && op_tab.size(1) == kOpCols,
              "op_tab must be int32 [n, 3]");
  TORCH_CHECK(xr_tab.dim() == 2 && xr_tab.size(1) == kXrCols,
              "xr_tab must be int64 [Rn, 8]");
  TORCH_CHECK(!lut.is_cuda() && lut.scalar_type() == at::kByte &&
                  lut.dim() == 1 && lut.numel() == 16 && lut.is_contiguous(),
              "lut must be a host uint8 [16] tensor");
  Lut l = {0, 0};
  const uint8_t* lp = lut.data_ptr<uint8_t>();
  for (int i = 0; i < 8; ++i) {
    l.lo |= (unsigned long long)lp[i] << (8 * i);
    l.hi |= (unsigned long long)lp[8 + i] << (8 * i);
  }
  ExpandSizes sz;
  sz.n_raw = raw.numel();
  sz.n_rows = op_tab.size(0);
  sz.n_src = src.numel();
  sz.Rn = (int)xr_tab.size(0);
  if (sz.Rn == 0) return;
  hipStream_t stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(
      cigar_expand_kernel, dim3((unsigned)sz.Rn), dim3(kThreads), 0, stream,
      raw.data_ptr<uint8_t>(), op_tab.data_ptr<int>(),
      reinterpret_cast<const long long*>(xr_tab.data_ptr<int64_t>()),
      src.data_ptr<uint8_t>(), l, sz);
}
