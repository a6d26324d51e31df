// Window-level QV calibration on device (K14 path + K15 compaction) for
// gfx950: which predicted base, carrying which QV, ended on a match, a
// mismatch or an insertion of the PBMM2-like alignment against truth.
//
// One 128-thread workgroup per example, three phases, all in LDS:
//   1. Compaction (K15): stable left shift of the non-gap positions of
//      label and bases (wave64 ballot + popcount prefix, the two waves
//      and the 128-column chunks stitched through LDS); every kept
//      predicted base remembers its window column.
//   2. Forward DP: the 3-state affine wavefront of metric_fwd_kernel
//      (alignment_metric.hip) -- same recurrences, same first-max tie
//      order (M, I, D), same fp32 arithmetic -- restricted to the
//      (sl+1) x (pl+1) cells the optimum and the backtrace can reach
//      (a cell depends only on cells with smaller i and j, so the cut
//      changes no value inside it). Directions are packed one byte per
//      cell (2 bits per state, 3 = invalid/stop) in an LDS table indexed
//      [i][j]; nothing of it goes to global memory.
//   3. Backtrace: lane 0 walks the path out of LDS, classifies each
//      predicted base (1 match, 2 mismatch, 3 insertion) at its window
//      column and bins it by QV into a per-workgroup LDS histogram,
//      which is flushed with at most one int64 atomic add per non-zero
//      bin (integer adds commute: the table is bitwise reproducible).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

namespace {

constexpr int CAL_MAXW = 160;  // max (L+1), as in alignment_metric.hip
constexpr int CAL_THREADS = 128;
constexpr int CAL_MAXQ = 100;  // calibrate's MAX_BASEQ
constexpr float CAL_NEG = -1e30f;
constexpr int DIR_STOP = 3;

// Row stride (bytes) of the direction table: cells of one anti-diagonal
// sit (stride - 1) bytes apart, so stride = 5 (mod 8) puts consecutive
// cells an odd number of dwords apart and spreads them over the banks.
__host__ __device__ inline int calib_dir_stride(int L) {
  int s = L + 1;
  while ((s & 7) != 5) ++s;
  return s;
}

// Fixed LDS carve (bytes); the direction table follows at CAL_FIXED.
constexpr int OFF_V = 0;                                 // f32 [3][3][MAXW]
constexpr int OFF_HIST = OFF_V + 3 * 3 * CAL_MAXW * 4;   // u32 [100][2]
constexpr int OFF_YT = OFF_HIST + CAL_MAXQ * 2 * 4;      // u8 [MAXW]
constexpr int OFF_YP = OFF_YT + CAL_MAXW;                // u8 [MAXW]
constexpr int OFF_PCOL = OFF_YP + CAL_MAXW;              // u8 [MAXW]
constexpr int OFF_Q = OFF_PCOL + CAL_MAXW;               // u8 [MAXW]
constexpr int OFF_CLS = OFF_Q + CAL_MAXW;                // u8 [MAXW]
constexpr int CAL_FIXED = OFF_CLS + CAL_MAXW;
static_assert(CAL_FIXED % 16 == 0, "direction table base alignment");

// Stable left shift of the non-zero entries of src[0..L) into dst,
// optionally recording each kept entry's column. Returns the kept count
// (block-uniform). s_wcnt: 2 ints of LDS scratch.
__device__ inline int compact_row(const uint8_t* __restrict__ src, int L,
                                  uint8_t* dst, uint8_t* dst_col,
                                  int* s_wcnt) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  int base = 0;
  for (int c0 = 0; c0 < L; c0 += CAL_THREADS) {
    const int col = c0 + tid;
    const uint8_t v = (col < L) ? src[col] : (uint8_t)0;
    const bool keep = v != 0;
    const unsigned long long mask = __ballot(keep);
    const int prefix = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) s_wcnt[wave] = __popcll(mask);
    __syncthreads();
    const int w0 = s_wcnt[0];
    const int w1 = s_wcnt[1];
    if (keep) {
      const int dst_i = base + (wave ? w0 : 0) + prefix;
      dst[dst_i] = v;
      if (dst_col) dst_col[dst_i] = (uint8_t)col;
    }
    base += w0 + w1;
    __syncthreads();
  }
  return base;
}

__global__ __launch_bounds__(CAL_THREADS) void alignment_calib_kernel(
    const uint8_t* __restrict__ label,  // [B, L] window coordinates
    const uint8_t* __restrict__ bases,  // [B, L]
    const uint8_t* __restrict__ quals,  // [B, L]
    float* __restrict__ v_opt,          // [B]
    int* __restrict__ counts,           // [B, 4]
    uint8_t* __restrict__ base_class,   // [B, L]
    unsigned long long* __restrict__ hist,  // [100, 2]
    int L, int stride,
    float ms, float mp, float go, float ge) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float (*vbuf)[3][CAL_MAXW] =
      reinterpret_cast<float (*)[3][CAL_MAXW]>(smem + OFF_V);
  unsigned int* s_hist = reinterpret_cast<unsigned int*>(smem + OFF_HIST);
  uint8_t* s_yt = reinterpret_cast<uint8_t*>(smem + OFF_YT);
  uint8_t* s_yp = reinterpret_cast<uint8_t*>(smem + OFF_YP);
  uint8_t* s_pcol = reinterpret_cast<uint8_t*>(smem + OFF_PCOL);
  uint8_t* s_q = reinterpret_cast<uint8_t*>(smem + OFF_Q);
  uint8_t* s_cls = reinterpret_cast<uint8_t*>(smem + OFF_CLS);
  uint8_t* s_dir = reinterpret_cast<uint8_t*>(smem + CAL_FIXED);
  __shared__ int s_wcnt[2];
  __shared__ float s_vopt;
  __shared__ int s_mopt;

  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const size_t row = (size_t)b * L;

  for (int i = tid; i < CAL_MAXQ * 2; i += CAL_THREADS) s_hist[i] = 0u;
  for (int i = tid; i < L; i += CAL_THREADS) {
    s_q[i] = quals[row + i];
    s_cls[i] = 0;
  }
  const int sl = compact_row(label + row, L, s_yt, nullptr, s_wcnt);
  const int pl = compact_row(bases + row, L, s_yp, s_pcol, s_wcnt);
  const int kend = sl + pl;

  float (*vm2)[CAL_MAXW] = vbuf[0];
  float (*vm1)[CAL_MAXW] = vbuf[1];
  float (*vcur)[CAL_MAXW] = vbuf[2];
  for (int i = tid; i <= sl; i += CAL_THREADS) {
    for (int s = 0; s < 3; ++s) {
      vm2[s][i] = CAL_NEG;
      vm1[s][i] = CAL_NEG;
    }
  }
  __syncthreads();
  if (tid == 0) {
    s_vopt = 0.f;
    s_mopt = -1;
    // k=0: V_M(0,0) = 0, start sentinel. k=1: V_I(0,1) = V_D(1,0) = -go,
    // both reached from M.
    vm2[0][0] = 0.f;
    s_dir[0] = (uint8_t)(DIR_STOP | (DIR_STOP << 2) | (DIR_STOP << 4));
    if (pl >= 1) {
      vm1[1][0] = -go;
      s_dir[1] = (uint8_t)(DIR_STOP | (0 << 2) | (DIR_STOP << 4));
    }
    if (sl >= 1) {
      vm1[2][1] = -go;
      s_dir[stride] = (uint8_t)(DIR_STOP | (DIR_STOP << 2) | (0 << 4));
    }
    if (kend == 1) {
      // At most one of the two k=1 cells exists; the other state is NEG.
      s_vopt = -go;
      s_mopt = (pl == 1) ? 1 : 2;
    }
  }
  __syncthreads();

  for (int k = 2; k <= kend; ++k) {
    const int ilo = max(0, k - pl);
    const int ihi = min(sl, k);
    for (int i = ilo + tid; i <= ihi; i += CAL_THREADS) {
      const int j = k - i;
      float vM = CAL_NEG, vI = CAL_NEG, vD = CAL_NEG;
      int dM = DIR_STOP, dI = DIR_STOP, dD = DIR_STOP;
      if (i >= 1 && j >= 1) {
        const float sub = (s_yt[i - 1] == s_yp[j - 1]) ? ms : -mp;
        // match: best state at (i-1, j-1).
        float best = vm2[0][i - 1];
        int bs = 0;
        if (vm2[1][i - 1] > best) { best = vm2[1][i - 1]; bs = 1; }
        if (vm2[2][i - 1] > best) { best = vm2[2][i - 1]; bs = 2; }
        if (best > CAL_NEG * 0.5f) {
          vM = best + sub;
          dM = bs;
        }
      }
      if (j >= 1) {
        // insertion: from M (-go) or I (-ge) at (i, j-1).
        const float cm = vm1[0][i] - go;
        const float ci = vm1[1][i] - ge;
        vI = cm;
        dI = 0;
        if (ci > vI) { vI = ci; dI = 1; }
        if (vI < CAL_NEG * 0.5f) { vI = CAL_NEG; dI = DIR_STOP; }
      }
      if (i >= 1) {
        // deletion: from M (-go), I (-go) or D (-ge) at (i-1, j).
        const float cm = vm1[0][i - 1] - go;
        const float ci = vm1[1][i - 1] - go;
        const float cd = vm1[2][i - 1] - ge;
        vD = cm;
        dD = 0;
        if (ci > vD) { vD = ci; dD = 1; }
        if (cd > vD) { vD = cd; dD = 2; }
        if (vD < CAL_NEG * 0.5f) { vD = CAL_NEG; dD = DIR_STOP; }
      }
      s_dir[i * stride + j] = (uint8_t)(dM | (dI << 2) | (dD << 4));
      vcur[0][i] = vM;
      vcur[1][i] = vI;
      vcur[2][i] = vD;
      if (k == kend && i == sl) {
        float best = vM;
        int bs = 0;
        if (vI > best) { best = vI; bs = 1; }
        if (vD > best) { best = vD; bs = 2; }
        s_vopt = best;
        s_mopt = bs;
      }
    }
    // One barrier per diagonal: diagonal k+1 overwrites the buffer that
    // diagonal k only read (vm2), and reads what k wrote. In-range cells
    // read in-range cells only, so stale entries are never consumed.
    __syncthreads();
    float (*t)[CAL_MAXW] = vm2;
    vm2 = vm1;
    vm1 = vcur;
    vcur = t;
  }

  if (tid == 0) {
    int i = sl, j = pl;
    int mc = s_mopt;
    int matches = 0, ins = 0, dels = 0, correct = 0;
    for (int step = 0; step <= kend; ++step) {
      if (mc < 0 || i < 0 || j < 0) break;
      const int mn = (s_dir[i * stride + j] >> (2 * mc)) & 3;
      if (mn == DIR_STOP) break;
      if (mc == 0) {
        const bool eq = s_yt[i - 1] == s_yp[j - 1];
        const int col = s_pcol[j - 1];
        ++matches;
        correct += eq ? 1 : 0;
        s_cls[col] = eq ? 1 : 2;
        const int q = s_q[col];
        if (q < CAL_MAXQ) s_hist[q * 2 + (eq ? 0 : 1)] += 1u;
        --i;
        --j;
      } else if (mc == 1) {
        const int col = s_pcol[j - 1];
        ++ins;
        s_cls[col] = 3;
        const int q = s_q[col];
        if (q < CAL_MAXQ) s_hist[q * 2 + 1] += 1u;
        --j;
      } else {
        ++dels;
        --i;
      }
      mc = mn;
    }
    v_opt[b] = s_vopt;
    counts[(size_t)b * 4 + 0] = matches;
    counts[(size_t)b * 4 + 1] = ins;
    counts[(size_t)b * 4 + 2] = dels;
    counts[(size_t)b * 4 + 3] = correct;
  }
  __syncthreads();

  for (int i = tid; i < L; i += CAL_THREADS) base_class[row + i] = s_cls[i];
  for (int i = tid; i < CAL_MAXQ * 2; i += CAL_THREADS) {
    const unsigned int c = s_hist[i];
    if (c) atomicAdd(hist + i, (unsigned long long)c);
  }
}

}  // namespace

size_t alignment_calib_lds_bytes(int64_t L) {
  const int stride = calib_dir_stride((int)L);
  return (size_t)CAL_FIXED + (size_t)(L + 1) * stride;
}

std::vector<at::Tensor> alignment_calib(
    at::Tensor label, at::Tensor bases, at::Tensor quals,
    double ms, double mp, double go, double ge) {
  TORCH_CHECK(label.is_cuda() && label.dtype() == at::kByte,
              "label uint8 cuda");
  TORCH_CHECK(bases.is_cuda() && bases.dtype() == at::kByte,
              "bases uint8 cuda");
  TORCH_CHECK(quals.is_cuda() && quals.dtype() == at::kByte,
              "quals uint8 cuda");
  TORCH_CHECK(label.dim() == 2, "label must be [B, L]");
  TORCH_CHECK(bases.sizes() == label.sizes() &&
              quals.sizes() == label.sizes(),
              "label, bases and quals must share one [B, L] shape");
  auto lc = label.contiguous();
  auto bc = bases.contiguous();
  auto qc = quals.contiguous();
  const int64_t B = lc.size(0), L = lc.size(1);
  TORCH_CHECK(L >= 1, "empty window");
  TORCH_CHECK(L + 1 < CAL_MAXW, "window too long for calibration kernel");
  auto v_opt = at::zeros({B}, lc.options().dtype(at::kFloat));
  auto counts = at::zeros({B, 4}, lc.options().dtype(at::kInt));
  auto base_class = at::zeros({B, L}, lc.options());
  auto hist = at::zeros({CAL_MAXQ, 2}, lc.options().dtype(at::kLong));
  if (B == 0) return {v_opt, counts, base_class, hist};
  const int stride = calib_dir_stride((int)L);
  const size_t lds = alignment_calib_lds_bytes(L);
  hipStream_t stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(
      alignment_calib_kernel, dim3((unsigned)B), dim3(CAL_THREADS), lds,
      stream, lc.data_ptr<uint8_t>(), bc.data_ptr<uint8_t>(),
      qc.data_ptr<uint8_t>(), v_opt.data_ptr<float>(),
      counts.data_ptr<int>(), base_class.data_ptr<uint8_t>(),
      reinterpret_cast<unsigned long long*>(hist.data_ptr<int64_t>()),
      (int)L, stride, (float)ms, (float)mp, (float)go, (float)ge);
  return {v_opt, counts, base_class, hist};
}
