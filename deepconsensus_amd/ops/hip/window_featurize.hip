// window_featurize — device-side window featurization.
//
// Expands compact per-ZMW planes into the int16 [N, R, L] model input
// (preprocess/featurize_device.py holds the packing, the host validator
// and the numpy twin; windows.py: iter_feature_dicts is the semantics):
//
//   sub    : uint8, per ZMW a row-major [3, n_sub, W] block (ids, pw, ip)
//   ccs    : uint8, per ZMW W CCS base ids
//   ccs_bq : int16, per ZMW W CCS qualities (read only with use_ccs_bq)
//   zmw_tab: int64 [Z, 5 + max_passes + 4] =
//            sub_off, ccs_off, bq_off, n_sub, W, strand[max_passes], sn[4]
//   win_tab: int32 [N, 3] = zmw_index, start, w
//
// Rows of window i, for n = min(n_sub, max_passes), columns c in [0, L):
//   f*mp + p      (f < 3)  sub[f][p][start + c]  for p < n, c < w, else 0
//   3*mp + p               strand[p]             for p < n (every column)
//   4*mp                   ccs[start + c]        for c < w, else 0
//   4*mp + 1   (use_bq)    ccs_bq[start + c]     for c < w, else -1
//   R-4 .. R-1             sn[k]                 if n > 0 (every column)
// A window with zmw_index outside [0, Z) is all zeros.
//
// Pure data movement, shaped around the stores: one workgroup per window,
// the window's R*L elements walked as one flat run, so consecutive lanes
// write consecutive addresses across row ends. A window is R*L*2 bytes;
// when L % 4 == 0 every row start stays 8-byte aligned and a lane stores
// 4 columns as one 8-byte vector, otherwise a lane stores one int16.
// Sources start at an arbitrary byte (`start` is arbitrary): byte loads,
// and 2-byte loads for ccs_bq. Table entries, strand and SN are uniform
// per window: read once into LDS.
//
// Every element of the output is written (zeros and -1 included), so the
// buffer needs no memset. Bounds: writes go to [i*R*L, (i+1)*R*L) for
// i < N only. Reads never trust the tables — a window whose ZMW's planes
// do not lie inside the source arrays is treated as zmw_index -1, n_sub is
// clamped to max_passes, start to [0, W], w to [0, min(L, W - start)].

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

namespace {

constexpr int kThreads = 256;
constexpr int kTabFixed = 5;

struct alignas(8) Short4 {
  short v[4];
};

// Uniform per-window state, filled by thread 0.
struct WindowInfo {
  long long sub_base;  // element offset of sub[0][0][start]
  long long ccs_base;  // element offset of ccs[start]
  long long bq_base;   // element offset of ccs_bq[start]
  long long plane;     // n_sub_raw * W: stride between the three planes
  long long W;
  int n_sub;  // clamped to max_passes; 0 also for an all-zero window
  int w;      // clamped; 0 for an all-zero window
  int live;   // 0: all-zero window
};

__device__ __forceinline__ short featurize_element(
    const uint8_t* __restrict__ sub, const uint8_t* __restrict__ ccs,
    const short* __restrict__ ccs_bq, const WindowInfo& info,
    const short* __restrict__ s_rowval, int r, int c, int mp, int use_bq,
    int sn_row0) {
  if (!info.live) return 0;
  if (r < 3 * mp) {
    const int f = r / mp;
    const int p = r - f * mp;
    if (p >= info.n_sub || c >= info.w) return 0;
    return (short)sub[info.sub_base + f * info.plane + p * info.W + c];
  }
  if (r < 4 * mp) return s_rowval[r - 3 * mp];  // strand, 0 for p >= n_sub
  if (r == 4 * mp) return c < info.w ? (short)ccs[info.ccs_base + c] : 0;
  if (r < sn_row0) {  // only reached with use_bq
    return c < info.w ? ccs_bq[info.bq_base + c] : (short)-1;
  }
  return s_rowval[mp + (r - sn_row0)];  // SN, 0 when n_sub == 0
}

// VEC columns per lane: 4 (8-byte stores, needs L % 4 == 0 and an 8-byte
// aligned output) or 1.
template <int VEC>
__global__ __launch_bounds__(kThreads) void window_featurize_kernel(
    const uint8_t* __restrict__ sub, const uint8_t* __restrict__ ccs,
    const short* __restrict__ ccs_bq, const long long* __restrict__ zmw_tab,
    const int* __restrict__ win_tab, short* __restrict__ out, int N, int Z,
    int R, int L, int mp, int use_bq, long long n_sub_bytes,
    long long n_ccs, long long n_bq) {
  extern __shared__ short s_rowval[];  // strand[mp], sn[4]
  __shared__ WindowInfo s_info;
  const int i = blockIdx.x;
  if (i >= N) return;
  const int n_col = kTabFixed + mp + 4;

  if (threadIdx.x == 0) {
    WindowInfo info = {};
    const int zi = win_tab[3 * i];
    if (zi >= 0 && zi < Z) {
      const long long* row = zmw_tab + (long long)zi * n_col;
      const long long sub_off = row[0], ccs_off = row[1], bq_off = row[2];
      const long long n_raw = row[3], W = row[4];
      // n_raw and W are bounded by the array sizes (< 2^31 each) before
      // they are multiplied.
      bool ok = n_raw >= 0 && W >= 0 && sub_off >= 0 && ccs_off >= 0 &&
                ccs_off <= n_ccs && W <= n_ccs - ccs_off &&
                sub_off <= n_sub_bytes && n_raw <= n_sub_bytes;
      if (ok) ok = n_raw * W <= (n_sub_bytes - sub_off) / 3;
      if (ok && use_bq) {
        ok = bq_off >= 0 && bq_off <= n_bq && W <= n_bq - bq_off;
      }
      if (ok) {
        long long start = win_tab[3 * i + 1];
        long long w = win_tab[3 * i + 2];
        start = start < 0 ? 0 : (start > W ? W : start);
        const long long room = W - start < L ? W - start : L;
        w = w < 0 ? 0 : (w > room ? room : w);
        info.live = 1;
        info.n_sub = (int)(n_raw < mp ? n_raw : mp);
        info.w = (int)w;
        info.W = W;
        info.plane = n_raw * W;
        info.sub_base = sub_off + start;
        info.ccs_base = ccs_off + start;
        info.bq_base = bq_off + start;
      }
    }
    s_info = info;
  }
  __syncthreads();
  const WindowInfo info = s_info;
  for (int k = threadIdx.x; k < mp + 4; k += kThreads) {
    short v = 0;
    if (info.live && info.n_sub > 0 && (k >= mp || k < info.n_sub)) {
      const int zi = win_tab[3 * i];
      v = (short)zmw_tab[(long long)zi * n_col + kTabFixed + k];
    }
    s_rowval[k] = v;
  }
  __syncthreads();

  const int sn_row0 = 4 * mp + 1 + (use_bq ? 1 : 0);
  const int per_row = L / VEC;  // lanes' units per row
  const int n_units = R * per_row;
  short* dst = out + (size_t)i * R * L;
  // Row/column of this lane's unit, advanced without a division per step.
  int r = threadIdx.x / per_row;
  int u = threadIdx.x - r * per_row;
  const int dr = kThreads / per_row;
  const int du = kThreads - dr * per_row;
  for (int e = threadIdx.x; e < n_units; e += kThreads) {
    const int c0 = u * VEC;
    if (VEC == 4) {
      Short4 q;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        q.v[k] = featurize_element(sub, ccs, ccs_bq, info, s_rowval, r,
                                   c0 + k, mp, use_bq, sn_row0);
      }
      *reinterpret_cast<Short4*>(dst + (size_t)r * L + c0) = q;
    } else {
      dst[(size_t)r * L + c0] = featurize_element(
          sub, ccs, ccs_bq, info, s_rowval, r, c0, mp, use_bq, sn_row0);
    }
    r += dr;
    u += du;
    if (u >= per_row) {
      u -= per_row;
      ++r;
    }
  }
}

void check_flat(const at::Tensor& t, at::ScalarType type, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a device tensor");
  TORCH_CHECK(t.scalar_type() == type, name, " must be ", type);
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.dim() == 1, name, " must be 1-D");
  TORCH_CHECK(t.numel() < (int64_t(1) << 31), name,
              " must be shorter than 2^31 elements");
}

void launch(const at::Tensor& sub, const at::Tensor& ccs,
            const at::Tensor& ccs_bq, const at::Tensor& zmw_tab,
            const at::Tensor& win_tab, at::Tensor& out, int64_t R,
            int64_t L, int64_t max_passes, bool use_ccs_bq) {
  check_flat(sub, at::kByte, "sub");
  check_flat(ccs, at::kByte, "ccs");
  check_flat(ccs_bq, at::kShort, "ccs_bq");
  TORCH_CHECK(max_passes >= 0 && max_passes <= 4096,
              "max_passes must be in 0..4096");
  TORCH_CHECK(L >= 1 && L <= (1 << 16), "L must be in 1..2^16");
  TORCH_CHECK(R == 4 * max_passes + 1 + (use_ccs_bq ? 1 : 0) + 4,
              "R must be 4 * max_passes + 5 (+ 1 with use_ccs_bq)");
  TORCH_CHECK(zmw_tab.is_cuda() && zmw_tab.scalar_type() == at::kLong &&
                  zmw_tab.is_contiguous() && zmw_tab.dim() == 2 &&
                  zmw_tab.size(1) == kTabFixed + max_passes + 4,
              "zmw_tab must be a contiguous int64 [Z, 5 + max_passes + 4] "
              "device tensor");
  TORCH_CHECK(win_tab.is_cuda() && win_tab.scalar_type() == at::kInt &&
                  win_tab.is_contiguous() && win_tab.dim() == 2 &&
                  win_tab.size(1) == 3,
              "win_tab must be a contiguous int32 [N, 3] device tensor");
  const int64_t N = win_tab.size(0);
  TORCH_CHECK(N < (int64_t(1) << 31) && zmw_tab.size(0) < (int64_t(1) << 31),
              "too many windows or ZMWs");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kShort &&
                  out.is_contiguous() && out.dim() == 3 &&
                  out.size(0) == N && out.size(1) == R && out.size(2) == L,
              "out must be a contiguous int16 [N, R, L] device tensor");
  TORCH_CHECK(ccs.device() == sub.device() &&
                  ccs_bq.device() == sub.device() &&
                  zmw_tab.device() == sub.device() &&
                  win_tab.device() == sub.device() &&
                  out.device() == sub.device(),
              "all tensors must be on the same device");
  if (N == 0) return;
  hipStream_t stream = at::hip::getCurrentHIPStream();
  const size_t lds = (size_t)(max_passes + 4) * sizeof(short);
  const bool vec4 =
      L % 4 == 0 && reinterpret_cast<uintptr_t>(out.data_ptr()) % 8 == 0;
  auto kernel =
      vec4 ? window_featurize_kernel<4> : window_featurize_kernel<1>;
  hipLaunchKernelGGL(
      kernel, dim3((unsigned)N), dim3(kThreads), lds, stream,
      sub.data_ptr<uint8_t>(), ccs.data_ptr<uint8_t>(),
      ccs_bq.data_ptr<short>(),
      reinterpret_cast<const long long*>(zmw_tab.data_ptr<int64_t>()),
      win_tab.data_ptr<int>(), out.data_ptr<short>(), (int)N,
      (int)zmw_tab.size(0), (int)R, (int)L, (int)max_passes,
      use_ccs_bq ? 1 : 0, (long long)sub.numel(), (long long)ccs.numel(),
      (long long)ccs_bq.numel());
}

}  // namespace

at::Tensor window_featurize(at::Tensor sub, at::Tensor ccs,
                            at::Tensor ccs_bq, at::Tensor zmw_tab,
                            at::Tensor win_tab, int64_t R, int64_t L,
                            int64_t max_passes, bool use_ccs_bq) {
  TORCH_CHECK(win_tab.dim() == 2, "win_tab must be [N, 3]");
  TORCH_CHECK(R >= 1 && L >= 1, "R and L must be positive");
  auto out = at::empty({win_tab.size(0), R, L},
                       sub.options().dtype(at::kShort));
  launch(sub, ccs, ccs_bq, zmw_tab, win_tab, out, R, L, max_passes,
         use_ccs_bq);
  return out;
}

// Same computation into a caller-owned int16 [N, R, L] tensor (possibly a
// view of a larger allocation); nothing outside it is written.
void window_featurize_into(at::Tensor sub, at::Tensor ccs,
                           at::Tensor ccs_bq, at::Tensor zmw_tab,
                           at::Tensor win_tab, at::Tensor out,
                           int64_t max_passes, bool use_ccs_bq) {
  TORCH_CHECK(out.dim() == 3, "out must be [N, R, L]");
  launch(sub, ccs, ccs_bq, zmw_tab, win_tab, out, out.size(1), out.size(2),
         max_passes, use_ccs_bq);
}
