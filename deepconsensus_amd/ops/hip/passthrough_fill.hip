// passthrough_fill — device-side CCS passthrough for skipped windows.
//
// A skipped window adopts the CCS bases and the (calibrated, clamped) CCS
// qualities of its columns. The planes of the featurize batch already hold
// both on the device, so a passthrough window is one table entry
// (preprocess/featurize_device.py holds the packing, the host validator and
// the numpy twin, passthrough_fill_numpy):
//
//   ccs     : uint8, per ZMW W CCS base ids
//   ccs_q   : uint8, per ZMW W CCS qualities coded q + 1 (0 = the -1 pad),
//             at the same offsets as ccs
//   zmw_tab : int64 [Z, ncol >= 5]; column 1 = ccs_off, column 4 = W
//   pt_tab  : int32 [P, 5] = zmw_index, start, w, width, dst_off
//   qual_lut: uint8 [256], code -> output QV (built on the host by the same
//             arithmetic as the host passthrough; no float math here)
//
// bases_out / quals_out are the passthrough region of the two rows of the
// stitch accumulation buffer, n bytes each. For entry i, c in [0, width):
//   bases_out[dst_off + c] = ccs[ccs_off + start + c]             c < w
//                            0                                    else
//   quals_out[dst_off + c] = qual_lut[ccs_q[ccs_off + start + c]] c < w
//                            qual_lut[0]                          else
// An entry with zmw_index outside [0, Z), or whose ZMW's planes do not lie
// inside ccs / ccs_q, is all id 0 / quality 0: all gap, dropped by the
// compaction. start is clamped to [0, W], w to [0, min(width, W - start)],
// a negative width counts as 0.
//
// Decomposition: the flat output range is walked, not the windows. A
// segment is 100 bytes in the common case, so one workgroup (or one wave)
// per window would idle most lanes and leave ragged 100-byte store runs;
// here consecutive lanes write consecutive dwords across segment ends and
// every wave store is one 256-byte run. Each lane owns one aligned dword
// of one output row (blockIdx.y: 0 bases, 1 quals) and finds the entry
// that owns each of its bytes by binary search over dst_off, narrowed
// first to the entries that meet the workgroup's 1 KiB span (that search
// depends on blockIdx only, so it is uniform). 4 bytes per lane rather
// than 16: the sources start at arbitrary bytes and are gathered bytewise
// either way. That the table lookups (a short search plus a six-load
// entry decode in front of every dword store) cost more than the narrow
// store is supposed, not measured: the kernel runs at 1.5-2.7x a
// device-to-device copy of the same bytes (~20 us per ZMW batch,
// profiles/r05_device_passthrough.md), and 16-byte lanes and a table
// slice staged in LDS per workgroup are untried.
//
// Stores: both rows start at arbitrary bytes (n_model * row_length is only
// a multiple of row_length, and the second row starts n_total further), so
// each row is cut at ITS OWN 4-byte boundaries: dword u covers addresses
// (row & ~3) + 4u .. + 3, which is aligned by construction. A dword whose
// four bytes are all owned is stored as one dword; the ragged first and
// last dword of the row (and any byte no entry owns) go bytewise.
// The LUT sits in LDS. No atomics.
//
// Bounds: a byte j is written only if 0 <= j < n and the entry found for
// it satisfies dst_off <= j < dst_off + width, so writes stay inside
// [dst_off, dst_off + width) and inside [0, n) whatever the tables hold. The search
// assumes dst_off ascending (the host validator enforces it); on a table
// that is not, some segments stay unwritten and nothing else happens.
// Every byte of every segment of a valid table is written: no memset.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

namespace {

constexpr int kThreads = 256;
constexpr int kTabFixed = 5;  // leading zmw_tab columns (window_featurize)
constexpr int kPtCols = 5;

// Decoded table entry, per lane.
struct Segment {
  long long off;  // dst_off
  long long end;  // dst_off + max(width, 0)
  long long src;  // ccs_off + start (clamped); valid when w > 0
  int w;          // clamped; 0 for a dead entry
  int live;       // 0: id 0 / quality 0 everywhere
};

// Largest i in [lo, hi] with dst_off[i] <= j, or lo when there is none.
__device__ __forceinline__ int find_entry(const int* __restrict__ pt_tab,
                                          int lo, int hi, long long j) {
  while (lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    if ((long long)pt_tab[(size_t)mid * kPtCols + 4] <= j) {
      lo = mid;
    } else {
      hi = mid - 1;
    }
  }
  return lo;
}

__device__ __forceinline__ Segment load_entry(
    const long long* __restrict__ zmw_tab, const int* __restrict__ pt_tab,
    int i, int Z, int n_col, long long n_ccs, long long n_q) {
  const int* e = pt_tab + (size_t)i * kPtCols;
  const int zi = e[0];
  const long long width = e[3] < 0 ? 0 : e[3];
  Segment s;
  s.off = e[4];
  s.end = s.off + width;
  s.src = 0;
  s.w = 0;
  s.live = 0;
  if (zi >= 0 && zi < Z) {
    const long long* row = zmw_tab + (size_t)zi * n_col;
    const long long ccs_off = row[1], W = row[4];
    const long long n_src = n_ccs < n_q ? n_ccs : n_q;
    if (ccs_off >= 0 && W >= 0 && ccs_off <= n_src && W <= n_src - ccs_off) {
      long long start = e[1];
      long long w = e[2];
      start = start < 0 ? 0 : (start > W ? W : start);
      const long long room = W - start < width ? W - start : width;
      w = w < 0 ? 0 : (w > room ? room : w);
      s.live = 1;
      s.w = (int)w;
      s.src = ccs_off + start;
    }
  }
  return s;
}

__global__ __launch_bounds__(kThreads) void passthrough_fill_kernel(
    const uint8_t* __restrict__ ccs, const uint8_t* __restrict__ ccs_q,
    const long long* __restrict__ zmw_tab, const int* __restrict__ pt_tab,
    const uint8_t* __restrict__ qual_lut, uint8_t* __restrict__ bases_out,
    uint8_t* __restrict__ quals_out, long long n, int P, int Z, int n_col,
    long long n_ccs, long long n_q) {
  __shared__ uint8_t s_lut[256];
  const int is_qual = blockIdx.y;
  s_lut[threadIdx.x] = qual_lut[threadIdx.x];  // kThreads == 256
  __syncthreads();

  const uint8_t* __restrict__ src_plane = is_qual ? ccs_q : ccs;
  uint8_t* out = is_qual ? quals_out : bases_out;
  const long long shift = (long long)(reinterpret_cast<uintptr_t>(out) & 3);
  const uint8_t pad = is_qual ? s_lut[0] : (uint8_t)0;

  // Entries that can own a byte of this workgroup's span (uniform).
  const long long span0 =
      (long long)blockIdx.x * (kThreads * 4) - shift;  // may be < 0
  const int e_lo = find_entry(pt_tab, 0, P - 1, span0);
  const int e_hi = find_entry(pt_tab, e_lo, P - 1, span0 + kThreads * 4 - 1);

  const long long j0 =
      ((long long)blockIdx.x * kThreads + threadIdx.x) * 4 - shift;
  if (j0 >= n) return;

  Segment seg;
  int cur = -1;
  uint8_t v[4];
  bool own[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long j = j0 + k;
    own[k] = false;
    v[k] = 0;
    if (j < 0 || j >= n) continue;
    if (cur < 0 || j < seg.off || j >= seg.end) {
      cur = find_entry(pt_tab, e_lo, e_hi, j);
      seg = load_entry(zmw_tab, pt_tab, cur, Z, n_col, n_ccs, n_q);
    }
    if (j < seg.off || j >= seg.end) continue;
    own[k] = true;
    const long long c = j - seg.off;
    if (!seg.live) {
      v[k] = 0;
    } else if (c < seg.w) {
      const uint8_t raw = src_plane[seg.src + c];
      v[k] = is_qual ? s_lut[raw] : raw;
    } else {
      v[k] = pad;
    }
  }
  if (own[0] && own[1] && own[2] && own[3]) {
    // All four in [0, n): out + j0 is the aligned dword (row & ~3) + 4u.
    const unsigned packed = (unsigned)v[0] | ((unsigned)v[1] << 8) |
                            ((unsigned)v[2] << 16) | ((unsigned)v[3] << 24);
    *reinterpret_cast<unsigned*>(out + j0) = packed;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (own[k]) out[j0 + k] = v[k];
    }
  }
}

void check_bytes(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a device tensor");
  TORCH_CHECK(t.scalar_type() == at::kByte, name, " must be uint8");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.dim() == 1, name, " must be 1-D");
  TORCH_CHECK(t.numel() < (int64_t(1) << 31), name,
              " must be shorter than 2^31 elements");
}

}  // namespace

void passthrough_fill_into(at::Tensor ccs, at::Tensor ccs_q,
                           at::Tensor zmw_tab, at::Tensor pt_tab,
                           at::Tensor qual_lut, at::Tensor bases_out,
                           at::Tensor quals_out) {
  check_bytes(ccs, "ccs");
  check_bytes(ccs_q, "ccs_q");
  check_bytes(qual_lut, "qual_lut");
  check_bytes(bases_out, "bases_out");
  check_bytes(quals_out, "quals_out");
  TORCH_CHECK(qual_lut.numel() == 256, "qual_lut must have 256 entries");
  TORCH_CHECK(bases_out.numel() == quals_out.numel(),
              "bases_out and quals_out must be of equal length");
  TORCH_CHECK(zmw_tab.is_cuda() && zmw_tab.scalar_type() == at::kLong &&
                  zmw_tab.is_contiguous() && zmw_tab.dim() == 2 &&
                  zmw_tab.size(1) >= kTabFixed,
              "zmw_tab must be a contiguous int64 [Z, >= 5] device tensor");
  TORCH_CHECK(pt_tab.is_cuda() && pt_tab.scalar_type() == at::kInt &&
                  pt_tab.is_contiguous() && pt_tab.dim() == 2 &&
                  pt_tab.size(1) == kPtCols,
              "pt_tab must be a contiguous int32 [P, 5] device tensor");
  const int64_t P = pt_tab.size(0);
  TORCH_CHECK(P < (int64_t(1) << 31) / kPtCols &&
                  zmw_tab.size(0) < (int64_t(1) << 31) &&
                  zmw_tab.size(1) < (int64_t(1) << 31),
              "too many windows, ZMWs or table columns");
  TORCH_CHECK(ccs_q.device() == ccs.device() &&
                  zmw_tab.device() == ccs.device() &&
                  pt_tab.device() == ccs.device() &&
                  qual_lut.device() == ccs.device() &&
                  bases_out.device() == ccs.device() &&
                  quals_out.device() == ccs.device(),
              "all tensors must be on the same device");
  const int64_t n = bases_out.numel();
  if (P == 0 || n == 0) return;
  // n + 3 < 2^31 + 3 bytes in dwords of 4, kThreads per workgroup.
  const int64_t n_dwords = (n + 3 + 3) / 4;
  const int64_t n_blocks = (n_dwords + kThreads - 1) / kThreads;
  hipStream_t stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(
      passthrough_fill_kernel, dim3((unsigned)n_blocks, 2), dim3(kThreads),
      0, stream, ccs.data_ptr<uint8_t>(), ccs_q.data_ptr<uint8_t>(),
      reinterpret_cast<const long long*>(zmw_tab.data_ptr<int64_t>()),
      pt_tab.data_ptr<int>(), qual_lut.data_ptr<uint8_t>(),
      bases_out.data_ptr<uint8_t>(), quals_out.data_ptr<uint8_t>(),
      (long long)n, (int)P, (int)zmw_tab.size(0), (int)zmw_tab.size(1),
      (long long)ccs.numel(), (long long)ccs_q.numel());
}
