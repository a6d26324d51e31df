// Distillation kernels (gfx950 / MI355X, wave64).
//
//  * ln_head_logits — final LayerNorm (eps 1e-6, fp32 statistics) + Dense(5)
//    head, emitting the fp32 logits that encode()["logits"] holds. Same
//    wave-per-position structure as fused_ln_head_qv_kernel (dc_kernels.hip):
//    per-lane LN and head weights in registers, persistent waves, next row
//    prefetched, two-pass variance. It stops before the softmax, so a frozen
//    teacher can run on the serving kernels and still hand logits to the
//    distillation loss.
//  * distill_loss_fwd — K17 in one pass: both temperature softmaxes, the
//    per-position KL or MSE term and the gradient with respect to the
//    student logits, semantics of models/losses.py DistillationLoss under
//    autograd (including both clamp_min(1e-12): a student probability below
//    the clamp passes no gradient through its log).
//
// The loss is a fixed-order two-stage sum in fp64 (per-block partials, then
// one block over the partials): no floating-point atomics, bitwise
// reproducible for a given M.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

using bf16 = __hip_bfloat16;

namespace {

// ---------------------------------------------------------------------------
// ln_head_logits
// ---------------------------------------------------------------------------
// Lane `lane` owns dims d = lane + 64*j, j < NS. One wave per position,
// 4 waves per block, grid-stride over positions.
template <typename T, int NS>
__global__ __launch_bounds__(256) void ln_head_logits_kernel(
    const T* __restrict__ x, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ w_head,
    const float* __restrict__ b_head, float* __restrict__ logits_out,
    int N, int H) {
  const int wave_in_block = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;

  float g[NS], bt[NS], wh[5][NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const int d = lane + 64 * j;
    g[j] = 0.f;
    bt[j] = 0.f;
#pragma unroll
    for (int k = 0; k < 5; ++k) wh[k][j] = 0.f;
    if (d < H) {
      g[j] = gamma[d];
      bt[j] = beta[d];
#pragma unroll
      for (int k = 0; k < 5; ++k) wh[k][j] = w_head[k * H + d];
    }
  }
  float bh[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) bh[k] = b_head[k];

  const int stride = gridDim.x * 4;
  int n = blockIdx.x * 4 + wave_in_block;
  T xr[NS];  // raw row, loaded one trip ahead
  if (n < N) {
    const T* xi = x + (size_t)n * H;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      const int d = lane + 64 * j;
      if (d < H) xr[j] = xi[d];
    }
  }
  for (; n < N; n += stride) {
    float sum = 0.f;
    float xv[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      xv[j] = 0.f;
      if (lane + 64 * j < H) {
        float v;
        if constexpr (std::is_same_v<T, bf16>) v = __bfloat162float(xr[j]);
        else v = xr[j];
        xv[j] = v;
        sum += v;
      }
    }
    if (n + stride < N) {
      const T* xi = x + (size_t)(n + stride) * H;
#pragma unroll
      for (int j = 0; j < NS; ++j) {
        const int d = lane + 64 * j;
        if (d < H) xr[j] = xi[d];
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    const float mean = sum / H;
    // Two-pass variance: sumsq/H - mean^2 cancels on near-constant rows.
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      if (lane + 64 * j < H) {
        const float dv = xv[j] - mean;
        sq += dv * dv;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sq += __shfl_xor(sq, off, 64);
    const float rstd = rsqrtf(sq / H + 1e-6f);

    float logit[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) logit[k] = 0.f;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      if (lane + 64 * j < H) {
        const float normed = (xv[j] - mean) * rstd * g[j] + bt[j];
#pragma unroll
        for (int k = 0; k < 5; ++k) logit[k] += normed * wh[k][j];
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
      for (int k = 0; k < 5; ++k) logit[k] += __shfl_xor(logit[k], off, 64);
    }
    // Every lane holds all five sums; lanes 0..4 store one logit each
    // (20 contiguous bytes per position).
    if (lane < 5) {
      float v = logit[0] + bh[0];
#pragma unroll
      for (int k = 1; k < 5; ++k)
        if (lane == k) v = logit[k] + bh[k];
      logits_out[(size_t)n * 5 + lane] = v;
    }
  }
}

// ---------------------------------------------------------------------------
// distill_loss_fwd
// ---------------------------------------------------------------------------
constexpr int DL_ROWS = 256;  // rows (= threads) per block
constexpr float DL_CLAMP = 1e-12f;

__device__ __forceinline__ void softmax5(const float* z, float temperature,
                                         float* p) {
  // softmax(z / T): torch divides by T, subtracts the row max, normalises.
  float v[5];
  float mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    v[k] = z[k] / temperature;
    mx = fmaxf(mx, v[k]);
  }
  float denom = 0.f;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    p[k] = expf(v[k] - mx);
    denom += p[k];
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) p[k] = p[k] / denom;
}

// One thread per position. The block's 256 x 5 logits are contiguous: they
// are staged through LDS with coalesced loads, and the gradient leaves the
// same way. A thread reads its row at stride 5 words (odd: no bank
// conflicts). partials[blockIdx.x] = the block's loss sum in fp64.
template <bool MSE>
__global__ __launch_bounds__(DL_ROWS) void distill_loss_kernel(
    const float* __restrict__ teacher, const float* __restrict__ student,
    float* __restrict__ grad, double* __restrict__ partials, long long M,
    float temperature, float grad_div) {
  __shared__ float sh_t[DL_ROWS * 5];
  __shared__ float sh_s[DL_ROWS * 5];
  __shared__ double sh_w[DL_ROWS / 64];

  const int tid = threadIdx.x;
  const long long row0 = (long long)blockIdx.x * DL_ROWS;
  const long long rows_here =
      (M - row0 < DL_ROWS) ? (M - row0) : (long long)DL_ROWS;
  const int n_el = (int)rows_here * 5;
  const float* tsrc = teacher + row0 * 5;
  const float* ssrc = student + row0 * 5;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int e = tid + i * DL_ROWS;
    if (e < n_el) {
      sh_t[e] = tsrc[e];
      sh_s[e] = ssrc[e];
    }
  }
  __syncthreads();

  double per = 0.0;
  float gr[5];
  const bool live = tid < rows_here;
  if (live) {
    float tl[5], sl[5], t[5], s[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      tl[k] = sh_t[tid * 5 + k];
      sl[k] = sh_s[tid * 5 + k];
    }
    softmax5(tl, temperature, t);
    softmax5(sl, temperature, s);
    float dz[5];
    if constexpr (MSE) {
      // per = mean_k (t - s)^2; dper/ds_k = -2 (t_k - s_k) / 5, then the
      // softmax Jacobian: dz_j = s_j (g_j - sum_k g_k s_k).
      float pp = 0.f;
      float gk[5];
      float c = 0.f;
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const float d = t[k] - s[k];
        pp += d * d;
        gk[k] = -2.f * d / 5.f;
        c += gk[k] * s[k];
      }
      per = (double)(pp / 5.f);
#pragma unroll
      for (int k = 0; k < 5; ++k) dz[k] = s[k] * (gk[k] - c);
    } else {
      // per = sum_k t_k (log max(t_k, c) - log max(s_k, c)), on the fp32
      // probabilities but with fp64 logs and products: against
      // log(1e-12) = -27.6 an fp32 log alone is off by up to 1e-6 per
      // term, more than the rounding of the fp32 result.
      // dper/ds_k = -t_k / s_k where s_k >= c, else 0, so through the
      // softmax Jacobian dz_j = s_j * A - [s_j >= c] t_j with
      // A = sum_{k: s_k >= c} t_k = 1 - (teacher mass on clamped classes):
      // exactly 1 when nothing is clamped.
      float clamped_mass = 0.f;
      bool pass[5];
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        pass[k] = s[k] >= DL_CLAMP;
        per += (double)t[k] * (log((double)fmaxf(t[k], DL_CLAMP)) -
                               log((double)fmaxf(s[k], DL_CLAMP)));
        if (!pass[k]) clamped_mass += t[k];
      }
      const float a = 1.f - clamped_mass;
#pragma unroll
      for (int k = 0; k < 5; ++k)
        dz[k] = s[k] * a - (pass[k] ? t[k] : 0.f);
    }
    // d(mean over M of per(z / T)) / d logits = dz / (T * M).
#pragma unroll
    for (int k = 0; k < 5; ++k) gr[k] = dz[k] / grad_div;
  }
  // A thread's own five sh_s slots now carry its gradient row; the barrier
  // below orders these writes before the coalesced copy-out.
  if (live) {
#pragma unroll
    for (int k = 0; k < 5; ++k) sh_s[tid * 5 + k] = gr[k];
  }

  // Block sum in fixed order: xor tree inside each wave, then waves 0..3.
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) per += __shfl_xor(per, off, 64);
  if ((tid & 63) == 0) sh_w[tid >> 6] = per;
  __syncthreads();
  if (tid == 0) {
    double acc = sh_w[0];
#pragma unroll
    for (int w = 1; w < DL_ROWS / 64; ++w) acc += sh_w[w];
    partials[blockIdx.x] = acc;
  }
  float* gdst = grad + row0 * 5;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int e = tid + i * DL_ROWS;
    if (e < n_el) gdst[e] = sh_s[e];
  }
}

// Second stage: one block sums the partials in a fixed order (thread t takes
// t, t + 256, ...; then the same tree) and writes loss = sum / M.
__global__ __launch_bounds__(DL_ROWS) void distill_loss_finish_kernel(
    const double* __restrict__ partials, int n_partials, long long M,
    float* __restrict__ loss) {
  __shared__ double sh_w[DL_ROWS / 64];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int i = tid; i < n_partials; i += DL_ROWS) acc += partials[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((tid & 63) == 0) sh_w[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double tot = sh_w[0];
#pragma unroll
    for (int w = 1; w < DL_ROWS / 64; ++w) tot += sh_w[w];
    loss[0] = (float)(tot / (double)M);
  }
}

}  // namespace

at::Tensor ln_head_logits(at::Tensor x, at::Tensor gamma, at::Tensor beta,
                          at::Tensor w_head, at::Tensor b_head,
                          c10::optional<at::Tensor> out) {
  TORCH_CHECK(x.is_cuda() && x.dim() >= 2, "x must be a device matrix");
  auto xc = x.contiguous();
  const int64_t H = xc.size(-1);
  TORCH_CHECK(H >= 1 && H <= 512, "H must be in 1..512");
  const int64_t N = xc.numel() / H;
  TORCH_CHECK(N < (int64_t(1) << 31), "too many positions");
  auto chk = [&](const at::Tensor& t, int64_t numel, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.dtype() == at::kFloat && t.numel() == numel,
                name, " must be a device fp32 tensor of ", numel,
                " elements");
  };
  chk(gamma, H, "gamma");
  chk(beta, H, "beta");
  chk(w_head, 5 * H, "w_head");
  chk(b_head, 5, "b_head");
  at::Tensor logits;
  if (out.has_value()) {
    logits = *out;
    TORCH_CHECK(logits.is_cuda() && logits.dtype() == at::kFloat &&
                    logits.is_contiguous() && logits.dim() == 2 &&
                    logits.size(0) == N && logits.size(1) == 5,
                "out must be a contiguous device fp32 [N, 5] tensor");
  } else {
    logits = at::empty({N, 5}, xc.options().dtype(at::kFloat));
  }
  if (N == 0) return logits;
  dim3 grid((unsigned)std::min<int64_t>((N + 3) / 4, 2048));
  dim3 block(256);
  hipStream_t stream = at::hip::getCurrentHIPStream();
  auto gc = gamma.contiguous(), bc = beta.contiguous();
  auto wc = w_head.contiguous(), bhc = b_head.contiguous();
  // Register slots per lane: 2, 5 (H = 280) or 8 cover every H <= 512.
  auto launch = [&](auto tag) {
    using T = decltype(tag);
    auto go = [&](auto kern) {
      hipLaunchKernelGGL(kern, grid, block, 0, stream,
                         reinterpret_cast<const T*>(xc.data_ptr()),
                         gc.data_ptr<float>(), bc.data_ptr<float>(),
                         wc.data_ptr<float>(), bhc.data_ptr<float>(),
                         logits.data_ptr<float>(), (int)N, (int)H);
    };
    if (H <= 128) go(ln_head_logits_kernel<T, 2>);
    else if (H <= 320) go(ln_head_logits_kernel<T, 5>);
    else go(ln_head_logits_kernel<T, 8>);
  };
  if (xc.dtype() == at::kBFloat16) {
    launch(bf16{});
  } else {
    TORCH_CHECK(xc.dtype() == at::kFloat, "x must be bf16 or fp32");
    launch(float{});
  }
  return logits;
}

std::vector<at::Tensor> distill_loss_fwd(at::Tensor teacher_logits,
                                         at::Tensor student_logits,
                                         double temperature, int64_t kind,
                                         c10::optional<at::Tensor> grad_out) {
  auto chk = [](const at::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.dtype() == at::kFloat && t.dim() >= 1 &&
                    t.size(-1) == 5,
                name, " must be a device fp32 [..., 5] tensor");
  };
  chk(teacher_logits, "teacher_logits");
  chk(student_logits, "student_logits");
  TORCH_CHECK(teacher_logits.numel() == student_logits.numel(),
              "teacher and student logits differ in size");
  TORCH_CHECK(kind == 0 || kind == 1, "kind: 0 = KL, 1 = MSE");
  TORCH_CHECK(temperature > 0, "temperature must be positive");
  auto tc = teacher_logits.contiguous();
  auto sc = student_logits.contiguous();
  const int64_t M = sc.numel() / 5;
  TORCH_CHECK(M >= 1, "no positions");
  const int64_t n_blocks = (M + DL_ROWS - 1) / DL_ROWS;
  TORCH_CHECK(n_blocks < (int64_t(1) << 31), "too many positions");
  at::Tensor grad;
  if (grad_out.has_value()) {
    grad = *grad_out;
    TORCH_CHECK(grad.is_cuda() && grad.dtype() == at::kFloat &&
                    grad.is_contiguous() && grad.numel() == M * 5,
                "grad_out must be a contiguous device fp32 [M, 5] tensor");
  } else {
    grad = at::empty_like(sc);
  }
  auto loss = at::empty({}, sc.options());
  auto partials = at::empty({n_blocks}, sc.options().dtype(at::kDouble));
  hipStream_t stream = at::hip::getCurrentHIPStream();
  const float t = (float)temperature;
  const float grad_div = t * (float)M;
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((unsigned)n_blocks), dim3(DL_ROWS), 0,
                       stream, tc.data_ptr<float>(), sc.data_ptr<float>(),
                       grad.data_ptr<float>(), partials.data_ptr<double>(),
                       (long long)M, t, grad_div);
  };
  if (kind == 1) go(distill_loss_kernel<true>);
  else go(distill_loss_kernel<false>);
  hipLaunchKernelGGL(distill_loss_finish_kernel, dim3(1), dim3(DL_ROWS), 0,
                     stream, partials.data_ptr<double>(), (int)n_blocks,
                     (long long)M, loss.data_ptr<float>());
  return {loss, grad};
}
