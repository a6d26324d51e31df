// subread_space — device-side subread spacing.
//
// Builds the spaced uint8 planes of a ZMW batch (the buffers that
// window_featurize and passthrough_fill read) from unspaced reads.
// preprocess/spacing_device.py holds the worker side, the packing, the host
// validator and the numpy twin (space_planes_numpy); read.py's spacing state
// machine is the semantics. The closed form, per ZMW with CCS length Lc:
//
//   an element of a read is an insertion (code bit 0x80) or consumes one
//   CCS position; ref(e) = non-insertion elements before e in its read,
//   k(e) = index of an insertion inside its run;
//   ins_max[c], c in 0..Lc = longest insertion run with ref == c over all
//   reads of the ZMW (computed by the worker);
//   col_ref[c] = c + sum(ins_max[0..c]);  slot0[c] = col_ref[c] - ins_max[c]
//   non-insertion -> column col_ref[ref];  insertion -> column slot0[ref] + k
//   W = Lc + sum(ins_max).
//
// Inputs (all caller-owned, flat unless a shape is given):
//   src     : uint8. Per kept read 3 * n bytes: codes[n] (base id, 0x80 on
//             an insertion), pw[n], ip[n]. Per ZMW 2 * Lc bytes: CCS base
//             ids[Lc], CCS quality codes q + 1 [Lc].
//   ins_max : uint16 (passed as int16 storage), per ZMW Lc + 1 entries
//   sp_tab  : int64 [S, 7] = zmw_index (row of zmw_tab), read0 (first row of
//             read_tab), n_reads, Lc, ins_off, ccs_src, flags (bit 0: write
//             the ZMW's ccs_q plane)
//   read_tab: int64 [Rn, 3] = sp_index, src_off, n
//   zmw_tab : int64 [Z, >= 5] = sub_off, ccs_off, bq_off, n_sub, W, ...
//   col_ref : int32 scratch, as long as ins_max, written by phase 1
// Outputs: sub (uint8, per ZMW [3, n_sub, W]), ccs, ccs_q (uint8, per ZMW W;
// ccs_q may be empty), ccs_bq (int16, per ZMW W; written with use_ccs_bq).
// The caller zero-fills the outputs: gap columns are not written, except in
// ccs_bq, whose gap columns are -1.
//
// Phase 1, one workgroup per sp_tab entry: inclusive scan of ins_max in
// tiles of kTile entries, the running sum carried from tile to tile in a
// register, so Lc is unbounded. The lane that owns position c stores
// col_ref[c], scatters the CCS row (ccs, ccs_q, ccs_bq) to column col_ref[c]
// and fills the ins_max[c] gap columns before it in ccs_bq with -1.
// Phase 2, one workgroup per read: a tiled add-scan of the non-insertion
// flag gives ref, a tiled max-scan of "index of the last non-insertion
// element" gives k, both carried across tiles; base id, pw and ip go to the
// read's row of the three planes. Phase 2 reads col_ref, so it is a second
// launch on the same stream.
//
// Within a wave the scans are shuffles over 64 lanes; the four wave totals
// of a workgroup go through LDS. Every column of a row is written by one
// lane only (columns of distinct elements of a read are distinct), so there
// are no atomics. Stores are single bytes (int16 for ccs_bq): the columns of
// consecutive elements are consecutive except at insertion slots, so a
// wave's byte stores still fall into few cache lines; wider stores would
// need a gather through LDS and are untried.
//
// Bounds: nothing is trusted. An sp_tab entry or read whose offsets do not
// lie inside src / ins_max / col_ref, whose zmw_index is outside [0, Z), or
// whose ZMW's planes do not lie inside the outputs is skipped whole. Every
// ref is clamped to [0, Lc], every column to [0, W), a read's row must be
// below n_sub. With a valid table (the host validator) no clamp acts.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

namespace {

constexpr int kThreads = 256;
constexpr int kTile = kThreads;  // one element per lane and tile
constexpr int kWaves = kThreads / 64;
constexpr int kSpCols = 7;
constexpr int kRdCols = 3;

// Inclusive workgroup scan of (add, mx) over the kThreads lanes; tot_add and
// tot_mx are the totals, the same in every lane. mx values are >= -1.
__device__ __forceinline__ void block_scan(int& add, int& mx, int* s_add,
                                           int* s_mx, int& tot_add,
                                           int& tot_mx) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int a = __shfl_up(add, d, 64);
    const int m = __shfl_up(mx, d, 64);
    if (lane >= d) {
      add += a;
      mx = mx > m ? mx : m;
    }
  }
  if (lane == 63) {
    s_add[wave] = add;
    s_mx[wave] = mx;
  }
  __syncthreads();
  int pre_add = 0, pre_mx = -1;
  tot_add = 0;
  tot_mx = -1;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const int a = s_add[w], m = s_mx[w];
    if (w < wave) {
      pre_add += a;
      pre_mx = pre_mx > m ? pre_mx : m;
    }
    tot_add += a;
    tot_mx = tot_mx > m ? tot_mx : m;
  }
  add += pre_add;
  mx = mx > pre_mx ? mx : pre_mx;
  __syncthreads();  // s_add / s_mx are rewritten by the next tile
}

// Uniform per-ZMW state, decoded identically by both phases.
struct ZmwInfo {
  long long Lc, ins_off, ccs_src, read0, n_reads;
  long long sub_off, ccs_off, bq_off, n_sub, W;
  bool want_q;
  bool ok;
};

struct Sizes {
  long long n_src, n_ins, n_sub_bytes, n_ccs, n_q, n_bq;
  int S, Rn, Z, n_col;
};

__device__ __forceinline__ ZmwInfo load_zmw(
    const long long* __restrict__ sp_tab,
    const long long* __restrict__ zmw_tab, long long s, const Sizes& sz) {
  ZmwInfo z = {};
  if (s < 0 || s >= sz.S) return z;
  const long long* e = sp_tab + s * kSpCols;
  const long long zi = e[0];
  z.read0 = e[1];
  z.n_reads = e[2];
  z.Lc = e[3];
  z.ins_off = e[4];
  z.ccs_src = e[5];
  z.want_q = (e[6] & 1) != 0;
  if (zi < 0 || zi >= sz.Z) return z;
  const long long* row = zmw_tab + zi * sz.n_col;
  z.sub_off = row[0];
  z.ccs_off = row[1];
  z.bq_off = row[2];
  z.n_sub = row[3];
  z.W = row[4];
  // Every size is < 2^31, so the sums below cannot overflow.
  bool ok = z.Lc >= 0 && z.Lc < sz.n_ins && z.ins_off >= 0 &&
            z.ins_off <= sz.n_ins - (z.Lc + 1);
  ok = ok && z.ccs_src >= 0 && z.ccs_src <= sz.n_src &&
       2 * z.Lc <= sz.n_src - z.ccs_src;
  ok = ok && z.W >= 1 && z.ccs_off >= 0 && z.ccs_off <= sz.n_ccs &&
       z.W <= sz.n_ccs - z.ccs_off;
  ok = ok && z.n_sub >= 0 && z.n_sub <= sz.n_sub_bytes && z.sub_off >= 0 &&
       z.sub_off <= sz.n_sub_bytes;
  if (ok) ok = z.n_sub * z.W <= (sz.n_sub_bytes - z.sub_off) / 3;
  z.ok = ok;
  return z;
}

__global__ __launch_bounds__(kThreads) void space_ccs_kernel(
    const uint8_t* __restrict__ src,
    const unsigned short* __restrict__ ins_max,
    const long long* __restrict__ sp_tab,
    const long long* __restrict__ zmw_tab, int* __restrict__ col_ref,
    uint8_t* __restrict__ ccs, uint8_t* __restrict__ ccs_q,
    short* __restrict__ ccs_bq, int use_bq, Sizes sz) {
  __shared__ int s_add[kWaves], s_mx[kWaves];
  const ZmwInfo z = load_zmw(sp_tab, zmw_tab, blockIdx.x, sz);
  if (!z.ok) return;  // uniform
  const bool q_ok = z.want_q && z.W <= sz.n_q - z.ccs_off;
  const bool bq_ok = use_bq && z.bq_off >= 0 && z.bq_off <= sz.n_bq &&
                     z.W <= sz.n_bq - z.bq_off;
  long long carry = 0;
  for (long long base = 0; base <= z.Lc; base += kTile) {
    const long long c = base + threadIdx.x;
    const int v = c <= z.Lc ? (int)ins_max[z.ins_off + c] : 0;
    int incl = v, unused = -1, tot, tot_mx;
    block_scan(incl, unused, s_add, s_mx, tot, tot_mx);
    if (c <= z.Lc) {
      long long col = c + carry + incl;
      col = col > z.W ? z.W : col;  // W = "one past the last column"
      col_ref[z.ins_off + c] = (int)col;
      if (c < z.Lc) {
        const long long cc = col > z.W - 1 ? z.W - 1 : col;
        const uint8_t q = src[z.ccs_src + z.Lc + c];
        ccs[z.ccs_off + cc] = src[z.ccs_src + c];
        if (q_ok) ccs_q[z.ccs_off + cc] = q;
        if (bq_ok) ccs_bq[z.bq_off + cc] = (short)((int)q - 1);
      }
      if (bq_ok) {
        long long g = col - v;
        g = g < 0 ? 0 : g;
        for (; g < col; ++g) ccs_bq[z.bq_off + g] = (short)-1;
      }
    }
    carry += tot;
  }
}

__global__ __launch_bounds__(kThreads) void space_reads_kernel(
    const uint8_t* __restrict__ src,
    const unsigned short* __restrict__ ins_max,
    const long long* __restrict__ sp_tab,
    const long long* __restrict__ read_tab,
    const long long* __restrict__ zmw_tab, const int* __restrict__ col_ref,
    uint8_t* __restrict__ sub, Sizes sz) {
  __shared__ int s_add[kWaves], s_mx[kWaves];
  const long long r = blockIdx.x;
  if (r >= sz.Rn) return;
  const long long* e = read_tab + r * kRdCols;
  const long long src_off = e[1], n = e[2];
  const ZmwInfo z = load_zmw(sp_tab, zmw_tab, e[0], sz);
  if (!z.ok) return;  // uniform, as every check below
  const long long row = r - z.read0;
  if (row < 0 || row >= z.n_reads || row >= z.n_sub) return;
  if (n < 0 || src_off < 0 || src_off > sz.n_src ||
      n > (sz.n_src - src_off) / 3) {
    return;
  }
  const long long plane = z.n_sub * z.W;
  const long long dst_row = z.sub_off + row * z.W;
  long long carry_ref = 0;
  long long carry_last = -1;
  for (long long base = 0; base < n; base += kTile) {
    const long long el = base + threadIdx.x;
    const bool active = el < n;
    const uint8_t code = active ? src[src_off + el] : (uint8_t)0x80;
    const int nonins = (active && !(code & 0x80)) ? 1 : 0;
    int incl = nonins;
    int last = nonins ? (int)threadIdx.x : -1;  // index inside the tile
    int tot, tot_last;
    block_scan(incl, last, s_add, s_mx, tot, tot_last);
    if (active) {
      long long ref = carry_ref + incl - nonins;
      ref = ref > z.Lc ? z.Lc : ref;
      long long col = col_ref[z.ins_off + ref];
      if (!nonins) {
        const long long last_el = last >= 0 ? base + last : carry_last;
        col = col - (long long)ins_max[z.ins_off + ref] + (el - 1 - last_el);
      }
      col = col < 0 ? 0 : (col > z.W - 1 ? z.W - 1 : col);
      const long long dst = dst_row + col;
      sub[dst] = code & 0x7f;
      sub[dst + plane] = src[src_off + n + el];
      sub[dst + 2 * plane] = src[src_off + 2 * n + el];
    }
    carry_ref += tot;
    if (tot_last >= 0) carry_last = base + tot_last;
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

int64_t subread_space_tile() { return kTile; }

void subread_space_into(at::Tensor src, at::Tensor ins_max,
                        at::Tensor sp_tab, at::Tensor read_tab,
                        at::Tensor zmw_tab, at::Tensor col_ref,
                        at::Tensor sub, at::Tensor ccs, at::Tensor ccs_q,
                        at::Tensor ccs_bq, bool use_ccs_bq) {
  check_dev(src, at::kByte, "src", src);
  check_dev(ins_max, at::kShort, "ins_max (uint16 as int16 storage)", src);
  check_dev(sp_tab, at::kLong, "sp_tab", src);
  check_dev(read_tab, at::kLong, "read_tab", src);
  check_dev(zmw_tab, at::kLong, "zmw_tab", src);
  check_dev(col_ref, at::kInt, "col_ref", src);
  check_dev(sub, at::kByte, "sub", src);
  check_dev(ccs, at::kByte, "ccs", src);
  check_dev(ccs_q, at::kByte, "ccs_q", src);
  check_dev(ccs_bq, at::kShort, "ccs_bq", src);
  for (const at::Tensor* t : {&src, &ins_max, &col_ref, &sub, &ccs, &ccs_q,
                              &ccs_bq}) {
    TORCH_CHECK(t->dim() == 1, "plane and source buffers must be 1-D");
  }
  TORCH_CHECK(sp_tab.dim() == 2 && sp_tab.size(1) == kSpCols,
              "sp_tab must be int64 [S, 7]");
  TORCH_CHECK(read_tab.dim() == 2 && read_tab.size(1) == kRdCols,
              "read_tab must be int64 [Rn, 3]");
  TORCH_CHECK(zmw_tab.dim() == 2 && zmw_tab.size(1) >= 5,
              "zmw_tab must be int64 [Z, >= 5]");
  TORCH_CHECK(col_ref.numel() == ins_max.numel(),
              "col_ref must be as long as ins_max");
  Sizes sz;
  sz.n_src = src.numel();
  sz.n_ins = ins_max.numel();
  sz.n_sub_bytes = sub.numel();
  sz.n_ccs = ccs.numel();
  sz.n_q = ccs_q.numel();
  sz.n_bq = ccs_bq.numel();
  sz.S = (int)sp_tab.size(0);
  sz.Rn = (int)read_tab.size(0);
  sz.Z = (int)zmw_tab.size(0);
  sz.n_col = (int)zmw_tab.size(1);
  if (sz.S == 0) return;
  hipStream_t stream = at::hip::getCurrentHIPStream();
  const unsigned short* ins_p =
      reinterpret_cast<const unsigned short*>(ins_max.data_ptr<int16_t>());
  const long long* sp_p =
      reinterpret_cast<const long long*>(sp_tab.data_ptr<int64_t>());
  const long long* zmw_p =
      reinterpret_cast<const long long*>(zmw_tab.data_ptr<int64_t>());
  hipLaunchKernelGGL(space_ccs_kernel, dim3((unsigned)sz.S), dim3(kThreads),
                     0, stream, src.data_ptr<uint8_t>(), ins_p, sp_p, zmw_p,
                     col_ref.data_ptr<int>(), ccs.data_ptr<uint8_t>(),
                     ccs_q.data_ptr<uint8_t>(), ccs_bq.data_ptr<int16_t>(),
                     use_ccs_bq ? 1 : 0, sz);
  if (sz.Rn == 0) return;
  hipLaunchKernelGGL(
      space_reads_kernel, dim3((unsigned)sz.Rn), dim3(kThreads), 0, stream,
      src.data_ptr<uint8_t>(), ins_p, sp_p,
      reinterpret_cast<const long long*>(read_tab.data_ptr<int64_t>()),
      zmw_p, col_ref.data_ptr<int>(), sub.data_ptr<uint8_t>(), sz);
}
