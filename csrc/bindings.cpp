// Python bindings for the tfosr gfx950 kernel set. Compiled with hipcc;
// kernels live in the .hip translation units and are reached through the
// extern "C" launchers so torch headers stay out of kernel code.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>
#include <c10/hip/HIPException.h>
#include <climits>
#include <map>
#include <mutex>

extern "C" {
int tfosr_bn_fast_blocks(long, int, int, int);
void tfosr_bn_apply_dual(const void*, const void*, void*, unsigned char*,
                         const float*, const float*, const float*, const float*,
                         const float*, const float*, const float*, const float*,
                         int, long, int, hipStream_t);
void tfosr_bn_bwd_stats_dual(const void*, const void*, const void*,
                             const unsigned char*, const float*, const float*,
                             const float*, const float*, float*, int, int, long,
                             int, hipStream_t);
void tfosr_bn_bwd_merge_dual(const float*, int, float*, float*, float*, float*,
                             int, hipStream_t);
void tfosr_bn_bwd_dx_dual(const void*, const void*, const void*,
                          const unsigned char*, void*, void*, const float*,
                          const float*, const float*, const float*, const float*,
                          const float*, const float*, const float*, const float*,
                          int, long, int, hipStream_t);
void tfosr_bn_stats(const void*, int, int, float*, int, int, int, long, hipStream_t);
void tfosr_bn_finalize(const float*, int, const void*, int, int, long,
                       float*, float*, float*, float*,
                       long, int, float, float, hipStream_t);
void tfosr_bn_apply(const void*, const void*, void*, unsigned char*,
                    const float*, const float*,
                    const float*, const float*, int, int, int, long, int, long,
                    hipStream_t);
void tfosr_bn_bwd_stats(const void*, const void*, const void*,
                        const unsigned char*, void*,
                        const float*, const float*, float*, int, int, int,
                        int, int, int, long, hipStream_t);
void tfosr_bn_bwd_merge(const float*, int, float*, float*, int, hipStream_t);
void tfosr_bn_bwd_dx(const void*, const void*, const void*,
                     const unsigned char*, const float*,
                     const float*, const float*, const float*, const float*,
                     void*, int, int, int, long, int, long, hipStream_t);
int tfosr_xent_dense_grid(int, int, long, long, int, int);
void tfosr_xent_dense_fwd(int, const void*, const long*, float*, float*, float*,
                          int*, int, long, long, int, long, float, int,
                          hipStream_t);
void tfosr_xent_dense_finalize(const float*, const int*, int, int, float*, int*,
                               hipStream_t);
void tfosr_xent_dense_bwd(int, const void*, const float*, const long*,
                          const float*, const float*, const int*, int, void*,
                          int, long, long, int, long, float, int, hipStream_t);
void tfosr_nhwc_pack(const void*, void*, const float*, const float*, float, int,
                     int, long, int, long, hipStream_t);
void tfosr_sgd_step(float*, const float*, float*, float, float, float, int, long,
                    hipStream_t);
void tfosr_adam_step(float*, const float*, float*, float*, float, float, float,
                     float, float, int, int, long, hipStream_t);
void tfosr_gemm_bt(const void*, const void*, void*, int, int, int, int,
                   hipStream_t);
void tfosr_gemm_bt_acc(const void*, const void*, void*, int, int, int, int,
                       int, hipStream_t);
void tfosr_mfma_probe(const short*, const short*, float*, hipStream_t);
void tfosr_maxpool_fwd(const void*, void*, unsigned char*, int, int, int, int,
                       int, int, int, int, int, int, hipStream_t);
void tfosr_maxpool_bwd(const void*, const unsigned char*, void*, int, int, int,
                       int, int, int, int, int, int, int, hipStream_t);
void tfosr_dwconv3x3_info(int*, int*, int*, int*, int*, int*, int*);
void tfosr_dwconv3x3_wrw_plan(long, int, int*, int*, int*, int*, long*);
void tfosr_dwconv3x3_fwd(const void*, const float*, void*, int, int, int, int,
                         int, int, int, int, hipStream_t);
void tfosr_dwconv3x3_dgrad(const void*, const float*, void*, int, int, int, int,
                           int, int, int, int, hipStream_t);
void tfosr_dwconv3x3_wrw(const void*, const void*, float*, float*, int, int,
                         int, int, int, int, int, int, hipStream_t);
void tfosr_conv3x3(const void*, const void*, const void*, void*, int, int, int,
                   int, int, int, int, int, int, int, hipStream_t);
void tfosr_conv_mfma(const void*, const void*, const void*, void*, int, int,
                     int, int, int, int, int, int, int, int, int, int, int,
                     int, int, hipStream_t);
int tfosr_conv3x3_halo_plan(int, int, int, int, int, int, int*, int*, long*,
                            long*, int*);
void tfosr_conv3x3_halo(const void*, const void*, void*, int, int, int, int,
                        int, int, hipStream_t);
void tfosr_conv_wrw(const void*, const void*, float*, int, int, int, int, int,
                    int, int, int, int, int, hipStream_t);
int tfosr_wrw2_split(int, int, long);
void tfosr_conv_wrw2(const void*, const void*, const void*, float*, float*,
                     int, int, int, int, int, int, int, int, int, int, int,
                     int, int, hipStream_t);
void tfosr_conv_stem(const void*, const void*, const void*, void*, int, int,
                     int, int, int, int, hipStream_t);
void tfosr_conv_par(const void*, const void*, const void*, void*, int, int,
                    int, int, int, int, int, int, int, unsigned long, int,
                    int, int, long, int, hipStream_t);
void tfosr_pack_bf16(const void*, const void*, int, void*, long, hipStream_t);
int tfosr_gemm_bt_stats_rows(int, int, int);
void tfosr_gemm_bt_stats(const void*, const void*, void*, float*, int, int, int,
                         hipStream_t);
void tfosr_conv_mfma_stats(const void*, const void*, const void*, void*, float*,
                           int, int, int, int, int, int, int, int, int, int, int,
                           int, hipStream_t);
int tfosr_bn_tile_ws_rows(int);
void tfosr_bn_tile_finalize(const float*, int, int, float*, float*, float*,
                            float*, float*, long, int, float, float,
                            hipStream_t);
}

namespace tfosr {
uint32_t crc32c(const uint8_t*, size_t, uint32_t);
struct ScanResult {
  std::string buffer;
  std::vector<std::pair<size_t, size_t>> records;
};
ScanResult scan_file(const std::string&, bool);
void write_file(const std::string&, const std::vector<std::string>&, bool);
}

namespace {

hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

// The conv kernels redirect out-of-image taps to a small all-zero buffer
// (every kernel takes it as const bf16_t* and only ever loads from it). One
// buffer per device, created on first use and kept for the process: it is
// zeroed with a blocking memset and a device synchronize before the pointer
// is handed out, so no stream can read it early, and later calls cost
// neither an allocation nor a fill launch.
const void* zero_guard(const at::Tensor& like) {
  constexpr size_t kGuardBytes = 256;  // kernels read at most 64 bf16
  static std::mutex mu;
  static std::map<int, void*> cache;
  TORCH_CHECK(like.is_cuda(), "zero_guard: expected a GPU tensor");
  const int dev = like.get_device();
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache.find(dev);
  if (it != cache.end()) return it->second;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  C10_HIP_CHECK(hipStreamIsCapturing(cur_stream(), &cap));
  TORCH_CHECK(cap == hipStreamCaptureStatusNone,
              "the conv kernels' zero guard for device ", dev,
              " is created on first use with a blocking fill, which a stream "
              "capture does not allow: run one conv on this device before "
              "capturing");
  int prev = 0;
  C10_HIP_CHECK(hipGetDevice(&prev));
  C10_HIP_CHECK(hipSetDevice(dev));
  void* p = nullptr;
  C10_HIP_CHECK(hipMalloc(&p, kGuardBytes));
  C10_HIP_CHECK(hipMemset(p, 0, kGuardBytes));
  C10_HIP_CHECK(hipDeviceSynchronize());
  C10_HIP_CHECK(hipSetDevice(prev));
  cache.emplace(dev, p);
  return p;
}

struct BNLayout {
  bool nhwc;
  int N, C;
  long HW;
};

BNLayout bn_layout(const at::Tensor& x) {
  TORCH_CHECK(x.dim() == 4, "expected 4-D NCHW tensor");
  BNLayout l;
  l.N = x.size(0);
  l.C = x.size(1);
  l.HW = (long)x.size(2) * x.size(3);
  if (x.is_contiguous(at::MemoryFormat::ChannelsLast)) {
    l.nhwc = true;
  } else {
    TORCH_CHECK(x.is_contiguous(), "input must be contiguous (NCHW or channels_last)");
    l.nhwc = false;
  }
  return l;
}

int dtype_flag(const at::Tensor& x) {
  TORCH_CHECK(x.is_cuda(), "bn: input must be a GPU tensor");
  if (x.scalar_type() == at::kBFloat16) return 1;
  TORCH_CHECK(x.scalar_type() == at::kFloat, "expected float32 or bfloat16");
  return 0;
}

// The launchers take raw pointers: everything they index is checked here.

// per-channel parameter / statistic: fp32, contiguous, length C, on x's device
void bn_check_channel_vec(const at::Tensor& t, const at::Tensor& x, int C,
                          const char* name) {
  TORCH_CHECK(t.device() == x.device(), "bn: ", name, " must be on ", x.device(),
              ", got ", t.device());
  TORCH_CHECK(t.scalar_type() == at::kFloat, "bn: ", name, " must be float32");
  TORCH_CHECK(t.dim() == 1 && t.size(0) == C, "bn: ", name,
              " must have shape [", C, "]");
  TORCH_CHECK(t.is_contiguous(), "bn: ", name, " must be contiguous");
}

// activation-shaped tensor: same sizes, dtype and device as x and, when
// same_layout is set, the same memory layout
void bn_check_like(const at::Tensor& t, const at::Tensor& x, bool nhwc,
                   bool same_layout, const char* name) {
  TORCH_CHECK(t.device() == x.device(), "bn: ", name, " must be on ", x.device(),
              ", got ", t.device());
  TORCH_CHECK(t.scalar_type() == x.scalar_type(), "bn: ", name,
              " must have the input's dtype");
  TORCH_CHECK(t.sizes() == x.sizes(), "bn: ", name,
              " must have the input's shape");
  if (same_layout) {
    TORCH_CHECK(nhwc ? t.is_contiguous(at::MemoryFormat::ChannelsLast)
                     : t.is_contiguous(),
                "bn: ", name, " must have the input's memory layout");
  }
}

std::vector<at::Tensor> bn_fwd_train(at::Tensor x, c10::optional<at::Tensor> res,
                                     at::Tensor w, at::Tensor b, at::Tensor rm,
                                     at::Tensor rv, double momentum, double eps,
                                     bool relu) {
  auto l = bn_layout(x);
  int bf = dtype_flag(x);
  const void* res_ptr = nullptr;
  if (res.has_value()) {
    bn_check_like(*res, x, l.nhwc, true, "res");
    res_ptr = res->data_ptr();
  }
  bn_check_channel_vec(w, x, l.C, "weight");
  bn_check_channel_vec(b, x, l.C, "bias");
  bn_check_channel_vec(rm, x, l.C, "running_mean");
  bn_check_channel_vec(rv, x, l.C, "running_var");
  auto opts = x.options().dtype(at::kFloat);
  long M = (long)l.N * l.HW;
  int nb = tfosr_bn_fast_blocks(M * l.C, l.C, bf, l.nhwc);
  auto ws = nb > 0 ? at::empty({(long)nb * 2 * l.C}, opts)
                   : at::zeros({2L * l.C}, opts);
  auto save_mean = at::empty({l.C}, opts);
  auto save_rstd = at::empty({l.C}, opts);
  auto y = at::empty_like(x);
  // relu sign bitmask (1 byte per vector) for y-free backward gating
  at::Tensor mask;
  unsigned char* mask_ptr = nullptr;
  if (relu && nb > 0) {
    long nvec = M * l.C / (bf ? 8 : 4);
    mask = at::empty({nvec}, x.options().dtype(at::kByte));
    mask_ptr = mask.data_ptr<unsigned char>();
  } else {
    mask = at::empty({0}, x.options().dtype(at::kByte));
  }
  auto s = cur_stream();
  tfosr_bn_stats(x.data_ptr(), bf, l.nhwc, ws.data_ptr<float>(), nb,
                 l.N, l.C, l.HW, s);
  tfosr_bn_finalize(ws.data_ptr<float>(), nb, x.data_ptr(), bf, l.nhwc, l.HW,
                    save_mean.data_ptr<float>(), save_rstd.data_ptr<float>(),
                    rm.data_ptr<float>(), rv.data_ptr<float>(), M, l.C,
                    (float)momentum, (float)eps, s);
  tfosr_bn_apply(x.data_ptr(), res_ptr, y.data_ptr(), mask_ptr,
                 save_mean.data_ptr<float>(),
                 save_rstd.data_ptr<float>(), w.data_ptr<float>(),
                 b.data_ptr<float>(), bf, l.nhwc, relu, M * l.C, l.C, l.HW, s);
  return {y, save_mean, save_rstd, mask};
}

at::Tensor bn_fwd_eval(at::Tensor x, c10::optional<at::Tensor> res, at::Tensor w,
                       at::Tensor b, at::Tensor rm, at::Tensor rv, double eps,
                       bool relu) {
  auto l = bn_layout(x);
  int bf = dtype_flag(x);
  const void* res_ptr = nullptr;
  if (res.has_value()) {
    bn_check_like(*res, x, l.nhwc, true, "res");
    res_ptr = res->data_ptr();
  }
  bn_check_channel_vec(w, x, l.C, "weight");
  bn_check_channel_vec(b, x, l.C, "bias");
  bn_check_channel_vec(rm, x, l.C, "running_mean");
  bn_check_channel_vec(rv, x, l.C, "running_var");
  auto rstd = at::rsqrt(rv + eps);
  auto y = at::empty_like(x);
  tfosr_bn_apply(x.data_ptr(), res_ptr, y.data_ptr(), nullptr,
                 rm.data_ptr<float>(),
                 rstd.data_ptr<float>(), w.data_ptr<float>(), b.data_ptr<float>(),
                 bf, l.nhwc, relu, (long)l.N * l.HW * l.C, l.C, l.HW,
                 cur_stream());
  return y;
}

std::vector<at::Tensor> bn_bwd(at::Tensor x, at::Tensor dy, at::Tensor y,
                               at::Tensor mask, at::Tensor w,
                               at::Tensor save_mean,
                               at::Tensor save_rstd, bool relu, bool grad_res) {
  auto l = bn_layout(x);
  int bf = dtype_flag(x);
  bn_check_like(dy, x, l.nhwc, false, "dy");
  bn_check_like(y, x, l.nhwc, true, "y");
  bn_check_channel_vec(w, x, l.C, "weight");
  bn_check_channel_vec(save_mean, x, l.C, "save_mean");
  bn_check_channel_vec(save_rstd, x, l.C, "save_rstd");
  dy = l.nhwc ? dy.contiguous(at::MemoryFormat::ChannelsLast) : dy.contiguous();
  auto opts = x.options().dtype(at::kFloat);
  long total = (long)l.N * l.HW * l.C;
  int nb = tfosr_bn_fast_blocks(total, l.C, bf, l.nhwc);
  auto ws = nb > 0 ? at::empty({(long)nb * 2 * l.C}, opts)
                   : at::zeros({2L * l.C}, opts);
  auto dg = at::empty({l.C}, opts);
  auto db = at::empty({l.C}, opts);
  auto dx = at::empty_like(x);
  at::Tensor gout;
  void* gout_ptr = nullptr;
  if (grad_res) {
    gout = at::empty_like(x);
    gout_ptr = gout.data_ptr();
  }
  auto s = cur_stream();
  const unsigned char* mask_ptr =
      mask.numel() ? mask.data_ptr<unsigned char>() : nullptr;
  TORCH_CHECK(!(relu && nb > 0) || mask_ptr != nullptr,
              "fast-path relu backward requires the forward bitmask");
  if (relu && nb > 0) {
    TORCH_CHECK(mask.device() == x.device() && mask.scalar_type() == at::kByte &&
                    mask.is_contiguous() && mask.numel() == total / (bf ? 8 : 4),
                "bn: mask must be the contiguous uint8 bitmask bn_fwd_train "
                "returned for this input");
  }
  tfosr_bn_bwd_stats(x.data_ptr(), dy.data_ptr(), y.data_ptr(), mask_ptr,
                     gout_ptr,
                     save_mean.data_ptr<float>(), save_rstd.data_ptr<float>(),
                     ws.data_ptr<float>(), nb, bf, l.nhwc,
                     relu, l.N, l.C, l.HW, s);
  tfosr_bn_bwd_merge(ws.data_ptr<float>(), nb, dg.data_ptr<float>(),
                     db.data_ptr<float>(), l.C, s);
  if (grad_res) {
    // gout already carries the gated gradient: skip re-gating (and the y read)
    tfosr_bn_bwd_dx(x.data_ptr(), gout.data_ptr(), y.data_ptr(), nullptr,
                    save_mean.data_ptr<float>(), save_rstd.data_ptr<float>(),
                    w.data_ptr<float>(), dg.data_ptr<float>(), db.data_ptr<float>(),
                    dx.data_ptr(), bf, l.nhwc, /*relu=*/0, total, l.C, l.HW, s);
    return {dx, dg, db, gout};
  }
  tfosr_bn_bwd_dx(x.data_ptr(), dy.data_ptr(), y.data_ptr(), mask_ptr,
                  save_mean.data_ptr<float>(), save_rstd.data_ptr<float>(),
                  w.data_ptr<float>(), dg.data_ptr<float>(), db.data_ptr<float>(),
                  dx.data_ptr(), bf, l.nhwc, relu, total, l.C, l.HW, s);
  return {dx, dg, db};
}

// The join of two training-mode BatchNorms, y = relu(bn_a(xa) + bn_b(xb)), on
// the NHWC fast path: the tail of a residual block with a downsample branch.
// bn_dual_eligible() says whether the dual entries take a pair; callers fall
// back to bn_fwd_train(xb) + bn_fwd_train(xa, res) and two bn_bwd otherwise.
bool bn_dual_eligible(const at::Tensor& xa, const at::Tensor& xb) {
  if (!xa.is_cuda() || !xb.is_cuda() || xa.dim() != 4) return false;
  if (xa.scalar_type() != at::kBFloat16 && xa.scalar_type() != at::kFloat)
    return false;
  if (xb.scalar_type() != xa.scalar_type() || xb.device() != xa.device() ||
      xb.sizes() != xa.sizes())
    return false;
  if (!xa.is_contiguous(at::MemoryFormat::ChannelsLast) ||
      !xb.is_contiguous(at::MemoryFormat::ChannelsLast))
    return false;
  return tfosr_bn_fast_blocks(xa.numel(), (int)xa.size(1),
                              xa.scalar_type() == at::kBFloat16, 1) > 0;
}

// -> {y, mean_a, rstd_a, mean_b, rstd_b, mask}; both running-stat pairs are
// updated. The statistics are those of bn_fwd_train (same kernels).
std::vector<at::Tensor> bn_dual_fwd_train(
    at::Tensor xa, at::Tensor xb, at::Tensor w_a, at::Tensor b_a,
    at::Tensor rm_a, at::Tensor rv_a, at::Tensor w_b, at::Tensor b_b,
    at::Tensor rm_b, at::Tensor rv_b, double momentum, double eps) {
  TORCH_CHECK(bn_dual_eligible(xa, xb),
              "bn_dual: needs two same-shape channels_last GPU tensors on the "
              "NHWC fast path");
  auto l = bn_layout(xa);
  int bf = dtype_flag(xa);
  const at::Tensor* vecs[] = {&w_a, &b_a, &rm_a, &rv_a, &w_b, &b_b, &rm_b, &rv_b};
  for (auto* t : vecs) bn_check_channel_vec(*t, xa, l.C, "per-channel vector");
  auto opts = xa.options().dtype(at::kFloat);
  long M = (long)l.N * l.HW;
  long total = M * l.C;
  int nb = tfosr_bn_fast_blocks(total, l.C, bf, 1);
  auto ws = at::empty({(long)nb * 2 * l.C}, opts);
  auto mean_a = at::empty({l.C}, opts), rstd_a = at::empty({l.C}, opts);
  auto mean_b = at::empty({l.C}, opts), rstd_b = at::empty({l.C}, opts);
  auto y = at::empty_like(xa);
  auto mask = at::empty({total / (bf ? 8 : 4)}, xa.options().dtype(at::kByte));
  auto s = cur_stream();
  auto f = [](at::Tensor& t) { return t.data_ptr<float>(); };
  // stream order lets the two statistics passes share one workspace
  tfosr_bn_stats(xa.data_ptr(), bf, 1, f(ws), nb, l.N, l.C, l.HW, s);
  tfosr_bn_finalize(f(ws), nb, xa.data_ptr(), bf, 1, l.HW, f(mean_a), f(rstd_a),
                    f(rm_a), f(rv_a), M, l.C, (float)momentum, (float)eps, s);
  tfosr_bn_stats(xb.data_ptr(), bf, 1, f(ws), nb, l.N, l.C, l.HW, s);
  tfosr_bn_finalize(f(ws), nb, xb.data_ptr(), bf, 1, l.HW, f(mean_b), f(rstd_b),
                    f(rm_b), f(rv_b), M, l.C, (float)momentum, (float)eps, s);
  tfosr_bn_apply_dual(xa.data_ptr(), xb.data_ptr(), y.data_ptr(),
                      mask.data_ptr<unsigned char>(), f(mean_a), f(rstd_a),
                      f(w_a), f(b_a), f(mean_b), f(rstd_b), f(w_b), f(b_b), bf,
                      total, l.C, s);
  return {y, mean_a, rstd_a, mean_b, rstd_b, mask};
}

// ---------------------------------------------------------------------------
// Batch statistics from the GEMM / conv epilogues: gemm_bt_stats and
// conv_mfma_stats return, next to the bf16 tensor, its per-tile partials
// part[ceil(M / rows_per_tile)][2][C] (csrc/mfma_stats_epilogue.h); the _pre
// entries below are bn_fwd_train / bn_dual_fwd_train with the statistics pass
// over the tensor replaced by a merge of those partials.
// ---------------------------------------------------------------------------

// x must be what the fast NHWC kernels take, in bf16 (the partials are those
// of a bf16 tensor); part must be the partials of a tensor of x's shape
void bn_check_pre(const at::Tensor& x, const BNLayout& l, const at::Tensor& part,
                  long rows_per_tile, const char* name) {
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && l.nhwc &&
                  tfosr_bn_fast_blocks(x.numel(), l.C, 1, 1) > 0,
              "bn_pre: needs a bfloat16 channels_last tensor on the NHWC fast "
              "path");
  TORCH_CHECK(part.device() == x.device(), "bn_pre: ", name, " must be on ",
              x.device(), ", got ", part.device());
  TORCH_CHECK(part.scalar_type() == at::kFloat, "bn_pre: ", name,
              " must be float32");
  TORCH_CHECK(part.is_contiguous(), "bn_pre: ", name, " must be contiguous");
  TORCH_CHECK(rows_per_tile >= 16 && rows_per_tile <= 4096,
              "bn_pre: bad rows_per_tile ", rows_per_tile);
  const long M = (long)l.N * l.HW;
  const long ntm = (M + rows_per_tile - 1) / rows_per_tile;
  TORCH_CHECK(part.dim() == 3 && part.size(0) == ntm && part.size(1) == 2 &&
                  part.size(2) == l.C,
              "bn_pre: ", name, " must have shape [", ntm, ", 2, ", l.C,
              "] for this input and rows_per_tile ", rows_per_tile);
}

void bn_tile_finalize(const at::Tensor& part, long rows_per_tile,
                      const BNLayout& l, at::Tensor& mean, at::Tensor& rstd,
                      at::Tensor& rm, at::Tensor& rv, double momentum,
                      double eps, hipStream_t s) {
  const int ntm = (int)part.size(0);
  auto ws = at::empty({(long)tfosr_bn_tile_ws_rows(ntm) * 3 * l.C},
                      part.options());
  tfosr_bn_tile_finalize(part.data_ptr<float>(), ntm, (int)rows_per_tile,
                         ws.data_ptr<float>(), mean.data_ptr<float>(),
                         rstd.data_ptr<float>(), rm.data_ptr<float>(),
                         rv.data_ptr<float>(), (long)l.N * l.HW, l.C,
                         (float)momentum, (float)eps, s);
}

// the statistics pass over x and its merge, as bn_fwd_train launches them on
// the NHWC fast path (nb = tfosr_bn_fast_blocks() > 0)
void bn_stats_pass(const at::Tensor& x, int bf, const BNLayout& l,
                   at::Tensor& mean, at::Tensor& rstd, at::Tensor& rm,
                   at::Tensor& rv, double momentum, double eps, hipStream_t s) {
  const long M = (long)l.N * l.HW;
  const int nb = tfosr_bn_fast_blocks(M * l.C, l.C, bf, 1);
  TORCH_CHECK(nb > 0, "bn: shape is not on the NHWC fast path");
  auto ws = at::empty({(long)nb * 2 * l.C}, x.options().dtype(at::kFloat));
  tfosr_bn_stats(x.data_ptr(), bf, 1, ws.data_ptr<float>(), nb, l.N, l.C, l.HW,
                 s);
  tfosr_bn_finalize(ws.data_ptr<float>(), nb, x.data_ptr(), bf, 1, l.HW,
                    mean.data_ptr<float>(), rstd.data_ptr<float>(),
                    rm.data_ptr<float>(), rv.data_ptr<float>(), M, l.C,
                    (float)momentum, (float)eps, s);
}

// -> what bn_fwd_train returns. Launches: tile merge, finalize, apply.
std::vector<at::Tensor> bn_fwd_train_pre(at::Tensor x,
                                         c10::optional<at::Tensor> res,
                                         at::Tensor part, long rows_per_tile,
                                         at::Tensor w, at::Tensor b,
                                         at::Tensor rm, at::Tensor rv,
                                         double momentum, double eps,
                                         bool relu) {
  auto l = bn_layout(x);
  dtype_flag(x);
  bn_check_pre(x, l, part, rows_per_tile, "part");
  const void* res_ptr = nullptr;
  if (res.has_value()) {
    bn_check_like(*res, x, true, true, "res");
    res_ptr = res->data_ptr();
  }
  bn_check_channel_vec(w, x, l.C, "weight");
  bn_check_channel_vec(b, x, l.C, "bias");
  bn_check_channel_vec(rm, x, l.C, "running_mean");
  bn_check_channel_vec(rv, x, l.C, "running_var");
  auto opts = x.options().dtype(at::kFloat);
  long total = (long)l.N * l.HW * l.C;
  auto save_mean = at::empty({l.C}, opts);
  auto save_rstd = at::empty({l.C}, opts);
  auto y = at::empty_like(x);
  at::Tensor mask = at::empty({relu ? total / 8 : 0},
                              x.options().dtype(at::kByte));
  auto s = cur_stream();
  bn_tile_finalize(part, rows_per_tile, l, save_mean, save_rstd, rm, rv,
                   momentum, eps, s);
  tfosr_bn_apply(x.data_ptr(), res_ptr, y.data_ptr(),
                 relu ? mask.data_ptr<unsigned char>() : nullptr,
                 save_mean.data_ptr<float>(), save_rstd.data_ptr<float>(),
                 w.data_ptr<float>(), b.data_ptr<float>(), 1, 1, relu, total,
                 l.C, l.HW, s);
  return {y, save_mean, save_rstd, mask};
}

// The statistics step of bn_fwd_train (part None: the pass over x and its
// merge) or of bn_fwd_train_pre (the tile merge) alone, without the apply:
// tools/bn_bench.py --epilogue times the two routes with it. -> {mean, rstd}
std::vector<at::Tensor> bn_batch_stats(at::Tensor x,
                                       c10::optional<at::Tensor> part,
                                       long rows_per_tile, at::Tensor rm,
                                       at::Tensor rv, double momentum,
                                       double eps) {
  auto l = bn_layout(x);
  int bf = dtype_flag(x);
  bn_check_channel_vec(rm, x, l.C, "running_mean");
  bn_check_channel_vec(rv, x, l.C, "running_var");
  auto opts = x.options().dtype(at::kFloat);
  auto mean = at::empty({l.C}, opts), rstd = at::empty({l.C}, opts);
  auto s = cur_stream();
  if (part.has_value()) {
    bn_check_pre(x, l, *part, rows_per_tile, "part");
    bn_tile_finalize(*part, rows_per_tile, l, mean, rstd, rm, rv, momentum,
                     eps, s);
    return {mean, rstd};
  }
  TORCH_CHECK(l.nhwc, "bn_batch_stats: expects a channels_last tensor");
  bn_stats_pass(x, bf, l, mean, rstd, rm, rv, momentum, eps, s);
  return {mean, rstd};
}

// -> what bn_dual_fwd_train returns. A branch given without partials (None:
// its producer had no statistics epilogue) gets the statistics pass.
std::vector<at::Tensor> bn_dual_fwd_train_pre(
    at::Tensor xa, at::Tensor xb, c10::optional<at::Tensor> part_a,
    long rows_a, c10::optional<at::Tensor> part_b, long rows_b,
    at::Tensor w_a, at::Tensor b_a, at::Tensor rm_a, at::Tensor rv_a,
    at::Tensor w_b, at::Tensor b_b, at::Tensor rm_b, at::Tensor rv_b,
    double momentum, double eps) {
  TORCH_CHECK(bn_dual_eligible(xa, xb),
              "bn_dual: needs two same-shape channels_last GPU tensors on the "
              "NHWC fast path");
  auto l = bn_layout(xa);
  TORCH_CHECK(xa.scalar_type() == at::kBFloat16,
              "bn_pre: needs bfloat16 tensors");
  if (part_a.has_value()) bn_check_pre(xa, l, *part_a, rows_a, "part_a");
  if (part_b.has_value()) bn_check_pre(xb, l, *part_b, rows_b, "part_b");
  const at::Tensor* vecs[] = {&w_a, &b_a, &rm_a, &rv_a, &w_b, &b_b, &rm_b, &rv_b};
  for (auto* t : vecs) bn_check_channel_vec(*t, xa, l.C, "per-channel vector");
  auto opts = xa.options().dtype(at::kFloat);
  long M = (long)l.N * l.HW;
  long total = M * l.C;
  auto mean_a = at::empty({l.C}, opts), rstd_a = at::empty({l.C}, opts);
  auto mean_b = at::empty({l.C}, opts), rstd_b = at::empty({l.C}, opts);
  auto y = at::empty_like(xa);
  auto mask = at::empty({total / 8}, xa.options().dtype(at::kByte));
  auto s = cur_stream();
  auto f = [](at::Tensor& t) { return t.data_ptr<float>(); };
  auto stats = [&](at::Tensor& x, c10::optional<at::Tensor>& part, long rows,
                   at::Tensor& mean, at::Tensor& rstd, at::Tensor& rm,
                   at::Tensor& rv) {
    if (part.has_value()) {
      bn_tile_finalize(*part, rows, l, mean, rstd, rm, rv, momentum, eps, s);
      return;
    }
    bn_stats_pass(x, 1, l, mean, rstd, rm, rv, momentum, eps, s);
  };
  stats(xa, part_a, rows_a, mean_a, rstd_a, rm_a, rv_a);
  stats(xb, part_b, rows_b, mean_b, rstd_b, rm_b, rv_b);
  tfosr_bn_apply_dual(xa.data_ptr(), xb.data_ptr(), y.data_ptr(),
                      mask.data_ptr<unsigned char>(), f(mean_a), f(rstd_a),
                      f(w_a), f(b_a), f(mean_b), f(rstd_b), f(w_b), f(b_b), 1,
                      total, l.C, s);
  return {y, mean_a, rstd_a, mean_b, rstd_b, mask};
}

// -> {dxa, dxb, dgamma_a, dgamma_b, dbeta_a, dbeta_b}; the two dbeta are the
// same sum (both BNs see the gated dy) in tensors of their own
std::vector<at::Tensor> bn_dual_bwd(at::Tensor xa, at::Tensor xb, at::Tensor dy,
                                    at::Tensor mask, at::Tensor w_a,
                                    at::Tensor mean_a, at::Tensor rstd_a,
                                    at::Tensor w_b, at::Tensor mean_b,
                                    at::Tensor rstd_b) {
  TORCH_CHECK(bn_dual_eligible(xa, xb),
              "bn_dual: needs two same-shape channels_last GPU tensors on the "
              "NHWC fast path");
  auto l = bn_layout(xa);
  int bf = dtype_flag(xa);
  bn_check_like(dy, xa, true, false, "dy");
  dy = dy.contiguous(at::MemoryFormat::ChannelsLast);
  const at::Tensor* vecs[] = {&w_a, &mean_a, &rstd_a, &w_b, &mean_b, &rstd_b};
  for (auto* t : vecs) bn_check_channel_vec(*t, xa, l.C, "per-channel vector");
  long total = (long)l.N * l.HW * l.C;
  TORCH_CHECK(mask.device() == xa.device() && mask.scalar_type() == at::kByte &&
                  mask.is_contiguous() && mask.numel() == total / (bf ? 8 : 4),
              "bn_dual: mask must be the contiguous uint8 bitmask "
              "bn_dual_fwd_train returned for these inputs");
  auto opts = xa.options().dtype(at::kFloat);
  int nb = tfosr_bn_fast_blocks(total, l.C, bf, 1);
  auto ws = at::empty({(long)nb * 3 * l.C}, opts);
  auto dg_a = at::empty({l.C}, opts), dg_b = at::empty({l.C}, opts);
  auto db_a = at::empty({l.C}, opts), db_b = at::empty({l.C}, opts);
  auto dxa = at::empty_like(xa), dxb = at::empty_like(xb);
  auto s = cur_stream();
  auto f = [](at::Tensor& t) { return t.data_ptr<float>(); };
  const unsigned char* mask_ptr = mask.data_ptr<unsigned char>();
  tfosr_bn_bwd_stats_dual(xa.data_ptr(), xb.data_ptr(), dy.data_ptr(), mask_ptr,
                          f(mean_a), f(rstd_a), f(mean_b), f(rstd_b), f(ws), nb,
                          bf, total, l.C, s);
  tfosr_bn_bwd_merge_dual(f(ws), nb, f(dg_a), f(dg_b), f(db_a), f(db_b), l.C, s);
  tfosr_bn_bwd_dx_dual(xa.data_ptr(), xb.data_ptr(), dy.data_ptr(), mask_ptr,
                       dxa.data_ptr(), dxb.data_ptr(), f(mean_a), f(rstd_a),
                       f(w_a), f(dg_a), f(mean_b), f(rstd_b), f(w_b), f(dg_b),
                       f(db_a), bf, total, l.C, s);
  return {dxa, dxb, dg_a, dg_b, db_a, db_b};
}

// One launch of one NHWC fast-path kernel family on caller-owned tensors, so
// that tools/bn_bench.py can time stats, apply, bwd stats and bwd dx apart
// (bn_fwd_train / bn_bwd run three launches each). family: 0 stats (x -> ws),
// 1 apply (x, other = res or none -> out, mask), 2 bwd stats (x, other = dy,
// mask -> ws, out = gout or none), 3 bwd dx (x, other = dy, mask -> out).
// p0..p3 are per-channel fp32 vectors: mean, rstd, weight, bias for apply;
// mean, rstd for bwd stats; mean, rstd, weight, dgamma for bwd dx with
// dbeta in p4. ws holds bn_fast_blocks() * 2C floats.
void bn_stage(int family, at::Tensor x, c10::optional<at::Tensor> other,
              c10::optional<at::Tensor> out, c10::optional<at::Tensor> mask,
              at::Tensor ws, std::vector<at::Tensor> p, bool relu) {
  auto l = bn_layout(x);
  int bf = dtype_flag(x);
  long total = (long)l.N * l.HW * l.C;
  int nb = tfosr_bn_fast_blocks(total, l.C, bf, l.nhwc);
  TORCH_CHECK(nb > 0, "bn_stage: shape is not on the NHWC fast path");
  const size_t need[4] = {0, 4, 2, 5};
  TORCH_CHECK(family >= 0 && family < 4, "bn_stage: family must be 0..3");
  TORCH_CHECK(p.size() == need[family], "bn_stage: family ", family, " takes ",
              need[family], " per-channel vectors");
  for (auto& t : p) bn_check_channel_vec(t, x, l.C, "per-channel vector");
  TORCH_CHECK(ws.device() == x.device() && ws.scalar_type() == at::kFloat &&
                  ws.is_contiguous() && ws.numel() >= (long)nb * 2 * l.C,
              "bn_stage: ws must hold bn_fast_blocks() * 2C floats");
  const void* other_ptr = nullptr;
  if (other.has_value()) {
    bn_check_like(*other, x, l.nhwc, true, "other");
    other_ptr = other->data_ptr();
  }
  void* out_ptr = nullptr;
  if (out.has_value()) {
    bn_check_like(*out, x, l.nhwc, true, "out");
    out_ptr = out->data_ptr();
  }
  unsigned char* mask_ptr = nullptr;
  if (mask.has_value()) {
    TORCH_CHECK(mask->device() == x.device() && mask->scalar_type() == at::kByte &&
                    mask->is_contiguous() && mask->numel() == total / (bf ? 8 : 4),
                "bn_stage: mask must be a contiguous uint8 tensor, one byte "
                "per 16 B vector");
    mask_ptr = mask->data_ptr<unsigned char>();
  }
  if (family != 0 && family != 1)
    TORCH_CHECK(other_ptr != nullptr, "bn_stage: dy is required");
  if (family == 1 || family == 3)
    TORCH_CHECK(out_ptr != nullptr, "bn_stage: out is required");
  if (family >= 2)
    TORCH_CHECK(!relu || mask_ptr != nullptr, "bn_stage: relu needs the mask");
  auto f = [&](size_t i) { return p[i].data_ptr<float>(); };
  auto s = cur_stream();
  switch (family) {
    case 0:
      tfosr_bn_stats(x.data_ptr(), bf, 1, ws.data_ptr<float>(), nb, l.N, l.C,
                     l.HW, s);
      break;
    case 1:
      tfosr_bn_apply(x.data_ptr(), other_ptr, out_ptr, mask_ptr, f(0), f(1),
                     f(2), f(3), bf, 1, relu, total, l.C, l.HW, s);
      break;
    case 2:
      tfosr_bn_bwd_stats(x.data_ptr(), other_ptr, nullptr, mask_ptr, out_ptr,
                         f(0), f(1), ws.data_ptr<float>(), nb, bf, 1, relu,
                         l.N, l.C, l.HW, s);
      break;
    default:
      tfosr_bn_bwd_dx(x.data_ptr(), other_ptr, nullptr, mask_ptr, f(0), f(1),
                      f(2), f(3), f(4), out_ptr, bf, 1, relu, total, l.C, l.HW,
                      s);
  }
}

// ---------------------------------------------------------------------------
// Dense softmax cross-entropy (csrc/softmax_xent_dense.hip)
// ---------------------------------------------------------------------------

enum { XENT_ROWS = 0, XENT_STRIDED = 1, XENT_TILE = 2 };
enum { XENT_NONE = 0, XENT_SUM = 1, XENT_MEAN = 2 };

// How the kernels see the logits: P rows or pixels of C classes; S is the
// class stride of the strided family (1 for class-contiguous rows).
struct XentLayout {
  int family;
  long P, S;
  int C;
};

// logits (P, C) with target (P,), or (N, C, d1, ...) with target
// (N, d1, ...). No layout makes a copy: class-contiguous rows (2-D, or 4-D
// channels_last through its flat view) go to the row-per-block kernels for
// C >= 64 and to the LDS-tile kernels below that; standard-contiguous N-D
// logits go to the class-strided kernels.
XentLayout xent_layout(const at::Tensor& logits, const at::Tensor& target) {
  TORCH_CHECK(logits.is_cuda(), "xent: logits must be a GPU tensor");
  TORCH_CHECK(logits.scalar_type() == at::kFloat ||
                  logits.scalar_type() == at::kBFloat16,
              "xent: logits must be float32 or bfloat16");
  TORCH_CHECK(logits.dim() >= 2, "xent: logits must be (P, C) or (N, C, d1, ...)");
  TORCH_CHECK(target.device() == logits.device(),
              "xent: target must be on ", logits.device());
  TORCH_CHECK(target.scalar_type() == at::kLong, "xent: target must be int64");
  TORCH_CHECK(target.is_contiguous(), "xent: target must be contiguous");
  TORCH_CHECK(target.dim() == logits.dim() - 1 &&
                  target.size(0) == logits.size(0),
              "xent: target must have the logits' shape without the class dim");
  for (int64_t d = 2; d < logits.dim(); ++d)
    TORCH_CHECK(target.size(d - 1) == logits.size(d),
                "xent: target must have the logits' shape without the class dim");
  TORCH_CHECK(logits.size(1) >= 1 && logits.size(1) < (1L << 24),
              "xent: bad class count");
  XentLayout l;
  l.C = (int)logits.size(1);
  l.P = target.numel();
  l.S = 1;
  bool rows;
  if (logits.dim() == 2) {
    TORCH_CHECK(logits.is_contiguous(), "xent: 2-D logits must be contiguous");
    rows = true;
  } else if (logits.is_contiguous()) {
    rows = false;
    for (int64_t d = 2; d < logits.dim(); ++d) l.S *= logits.size(d);
  } else {
    TORCH_CHECK(logits.dim() == 4 &&
                    logits.is_contiguous(at::MemoryFormat::ChannelsLast),
                "xent: N-D logits must be contiguous or 4-D channels_last");
    rows = true;
  }
  l.family = rows ? (l.C >= 64 ? XENT_ROWS : XENT_TILE) : XENT_STRIDED;
  return l;
}

void xent_check_rowvec(const at::Tensor& t, const at::Tensor& logits, long P,
                       const char* name) {
  TORCH_CHECK(t.device() == logits.device() && t.scalar_type() == at::kFloat &&
                  t.is_contiguous() && t.numel() == P,
              "xent: ", name, " must be contiguous float32 with one value per "
              "row, on the logits' device");
}

// reduction 0 none / 1 sum / 2 mean. Returns {loss, lse, n_valid}: loss has
// the target's shape for none and is a 0-dim device scalar otherwise;
// n_valid (int32[1], device) is empty for none. max_grid 0 = project cap.
std::vector<at::Tensor> xent_dense_fwd(at::Tensor logits, at::Tensor target,
                                       long ignore_index, double label_smoothing,
                                       long reduction, long max_grid) {
  auto l = xent_layout(logits, target);
  TORCH_CHECK(reduction >= XENT_NONE && reduction <= XENT_MEAN,
              "xent: reduction must be 0 (none), 1 (sum) or 2 (mean)");
  TORCH_CHECK(label_smoothing >= 0.0 && label_smoothing <= 1.0,
              "xent: label_smoothing must be in [0, 1]");
  TORCH_CHECK(max_grid >= 0, "xent: max_grid must be >= 0");
  int bf = dtype_flag(logits);
  auto fopts = logits.options().dtype(at::kFloat);
  auto iopts = logits.options().dtype(at::kInt);
  auto lse = at::empty({l.P}, fopts);
  auto s = cur_stream();
  if (reduction == XENT_NONE) {
    auto loss = at::empty(target.sizes(), fopts);
    tfosr_xent_dense_fwd(l.family, logits.data_ptr(), target.data_ptr<long>(),
                         loss.data_ptr<float>(), lse.data_ptr<float>(), nullptr,
                         nullptr, bf, l.P, l.S, l.C, ignore_index,
                         (float)label_smoothing, (int)max_grid, s);
    return {loss, lse, at::empty({0}, iopts)};
  }
  auto loss = at::zeros({}, fopts);
  auto nvalid = at::zeros({1}, iopts);
  if (l.P > 0) {
    int nb = tfosr_xent_dense_grid(l.family, bf, l.P, l.S, l.C, (int)max_grid);
    auto part_loss = at::empty({2L * nb}, fopts);
    auto part_cnt = at::empty({nb}, iopts);
    tfosr_xent_dense_fwd(l.family, logits.data_ptr(), target.data_ptr<long>(),
                         nullptr, lse.data_ptr<float>(),
                         part_loss.data_ptr<float>(), part_cnt.data_ptr<int>(),
                         bf, l.P, l.S, l.C, ignore_index,
                         (float)label_smoothing, (int)max_grid, s);
    tfosr_xent_dense_finalize(part_loss.data_ptr<float>(),
                              part_cnt.data_ptr<int>(), nb,
                              reduction == XENT_MEAN, loss.data_ptr<float>(),
                              nvalid.data_ptr<int>(), s);
  }
  return {loss, lse, nvalid};
}

// gout: per-row upstream gradient (none, the target's shape) or a one-element
// device scalar (sum / mean, with the forward's n_valid).
at::Tensor xent_dense_bwd(at::Tensor logits, at::Tensor lse, at::Tensor target,
                          at::Tensor gout, c10::optional<at::Tensor> nvalid,
                          long ignore_index, double label_smoothing,
                          long reduction, long max_grid) {
  auto l = xent_layout(logits, target);
  TORCH_CHECK(reduction >= XENT_NONE && reduction <= XENT_MEAN,
              "xent: reduction must be 0 (none), 1 (sum) or 2 (mean)");
  TORCH_CHECK(max_grid >= 0, "xent: max_grid must be >= 0");
  int bf = dtype_flag(logits);
  xent_check_rowvec(lse, logits, l.P, "lse");
  const float* grows = nullptr;
  const float* gscalar = nullptr;
  const int* nv = nullptr;
  if (reduction == XENT_NONE) {
    xent_check_rowvec(gout, logits, l.P, "gout");
    grows = gout.data_ptr<float>();
  } else {
    TORCH_CHECK(gout.device() == logits.device() &&
                    gout.scalar_type() == at::kFloat && gout.numel() == 1,
                "xent: gout must be a one-element float32 device tensor");
    TORCH_CHECK(nvalid.has_value() && nvalid->device() == logits.device() &&
                    nvalid->scalar_type() == at::kInt && nvalid->numel() == 1,
                "xent: n_valid must be the int32[1] tensor the forward returned");
    gscalar = gout.data_ptr<float>();
    nv = nvalid->data_ptr<int>();
  }
  // same sizes and strides as the logits
  auto dlogits = at::empty_like(logits);
  tfosr_xent_dense_bwd(l.family, logits.data_ptr(), lse.data_ptr<float>(),
                       target.data_ptr<long>(), grows, gscalar, nv,
                       reduction == XENT_MEAN, dlogits.data_ptr(), bf, l.P, l.S,
                       l.C, ignore_index, (float)label_smoothing, (int)max_grid,
                       cur_stream());
  return dlogits;
}

// Plain 2-D entry points for callers of the extension: per-row loss, no
// ignore_index or smoothing, row-per-block kernels for every C.
std::vector<at::Tensor> softmax_xent_fwd(at::Tensor logits, at::Tensor target) {
  TORCH_CHECK(logits.dim() == 2 && logits.is_contiguous());
  TORCH_CHECK(target.scalar_type() == at::kLong && target.is_cuda() &&
              target.is_contiguous() && target.numel() == logits.size(0));
  long N = logits.size(0);
  int C = logits.size(1);
  auto opts = logits.options().dtype(at::kFloat);
  auto loss = at::empty({N}, opts);
  auto lse = at::empty({N}, opts);
  tfosr_xent_dense_fwd(XENT_ROWS, logits.data_ptr(), target.data_ptr<long>(),
                       loss.data_ptr<float>(), lse.data_ptr<float>(), nullptr,
                       nullptr, dtype_flag(logits), N, 1, C, -100, 0.f, 0,
                       cur_stream());
  return {loss, lse};
}

at::Tensor softmax_xent_bwd(at::Tensor logits, at::Tensor lse, at::Tensor target,
                            at::Tensor gout) {
  TORCH_CHECK(logits.dim() == 2 && logits.is_contiguous());
  TORCH_CHECK(target.scalar_type() == at::kLong && target.is_cuda() &&
              target.is_contiguous() && target.numel() == logits.size(0));
  long N = logits.size(0);
  int C = logits.size(1);
  gout = gout.contiguous();
  xent_check_rowvec(lse, logits, N, "lse");
  xent_check_rowvec(gout, logits, N, "gout");
  auto dlogits = at::empty_like(logits);
  tfosr_xent_dense_bwd(XENT_ROWS, logits.data_ptr(), lse.data_ptr<float>(),
                       target.data_ptr<long>(), gout.data_ptr<float>(), nullptr,
                       nullptr, 0, dlogits.data_ptr(), dtype_flag(logits), N, 1,
                       C, -100, 0.f, 0, cur_stream());
  return dlogits;
}

at::Tensor nhwc_pack(at::Tensor x, at::Tensor mean, at::Tensor std_, double scale,
                     bool out_bf16, bool channels_last) {
  TORCH_CHECK(x.dim() == 4 && x.scalar_type() == at::kByte && x.is_contiguous(),
              "nhwc_pack expects contiguous uint8 NHWC");
  TORCH_CHECK(x.is_cuda(), "nhwc_pack: images must be on the GPU");
  for (int d = 0; d < 4; ++d)
    TORCH_CHECK(x.size(d) <= INT_MAX, "nhwc_pack: dimension ", d, " too large");
  int N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  long HW = (long)H * W;
  // the kernels index mean[c] / std_[c] for c < C through raw float pointers
  auto check_stat = [&](const at::Tensor& t, const char* name) {
    TORCH_CHECK(t.scalar_type() == at::kFloat && t.is_contiguous() &&
                    t.device() == x.device() && t.numel() == C,
                "nhwc_pack: ", name, " must be a contiguous fp32 tensor of C = ",
                C, " elements on the images' device");
  };
  check_stat(mean, "mean");
  check_stat(std_, "std");
  auto opts = x.options().dtype(out_bf16 ? at::kBFloat16 : at::kFloat);
  at::Tensor out;
  if (channels_last) {
    out = at::empty({N, C, H, W}, opts, at::MemoryFormat::ChannelsLast);
  } else {
    out = at::empty({N, C, H, W}, opts);
  }
  tfosr_nhwc_pack(x.data_ptr(), out.data_ptr(), mean.data_ptr<float>(),
                  std_.data_ptr<float>(), (float)scale, out_bf16, channels_last,
                  (long)N * C * HW, C, HW, cur_stream());
  return out;
}

// The flat optimizer kernels walk raw float pointers over p.numel() elements
// of every state tensor: all of them fp32, contiguous, equally long and on
// p's GPU.
void check_flat_state(const char* op, const at::Tensor& p,
                      std::initializer_list<const at::Tensor*> others) {
  TORCH_CHECK(p.is_cuda() && p.scalar_type() == at::kFloat && p.is_contiguous(),
              op, " expects contiguous fp32 params on the GPU");
  for (const at::Tensor* t : others)
    TORCH_CHECK(t->scalar_type() == at::kFloat && t->is_contiguous() &&
                    t->device() == p.device() && t->numel() == p.numel(),
                op, ": every tensor must be contiguous fp32 with the params' ",
                p.numel(), " elements on the params' device");
}

// Shared max-pool argument checks. The kernels index threads with u32 and
// store the window tap in a u8; returns {OH, OW}.
std::pair<long, long> check_pool_geometry(const char* op, const at::Tensor& t,
                                          long C, long N, long H, long W,
                                          long K, long S, long P) {
  TORCH_CHECK(t.is_cuda(), op, " expects a GPU tensor");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16 || t.scalar_type() == at::kFloat,
              op, " expects bf16 or fp32");
  const long V = t.scalar_type() == at::kBFloat16 ? 8 : 4;
  TORCH_CHECK(C >= V && C % V == 0, op, ": C must be a multiple of ", V,
              " for this dtype, got ", C);
  TORCH_CHECK(K >= 1 && S >= 1 && K * K <= 256, op,
              ": need K >= 1, S >= 1 and K*K <= 256 (the saved tap index is "
              "one byte), got K=", K, " S=", S);
  TORCH_CHECK(P >= 0 && P <= K / 2, op, ": need 0 <= P <= K/2, got P=", P);
  TORCH_CHECK(N >= 0 && H >= 1 && W >= 1 && H <= INT_MAX && W <= INT_MAX &&
              N <= INT_MAX && C <= INT_MAX && S <= INT_MAX,
              op, ": empty or oversized dimension");
  TORCH_CHECK(H + 2 * P >= K && W + 2 * P >= K, op,
              ": the window does not fit the padded input");
  const long OH = (H + 2 * P - K) / S + 1, OW = (W + 2 * P - K) / S + 1;
  // one thread per V channels of a pixel, u32 index advanced by grid-stride:
  // keep count + stride below 2^32 (no overflow in the products: each
  // factor is below 2^31 and the running product is checked as it grows)
  const long limit = 0xFFFFFFFFL - 2048L * 256L;
  auto fits = [&](long h, long w) {
    long n = N;
    for (long f : {h, w, C / V}) {
      if (n > limit / f) return false;
      n *= f;
    }
    return true;
  };
  TORCH_CHECK(fits(H, W) && fits(OH, OW), op,
              ": tensor too large for the kernels' 32-bit thread index");
  return {OH, OW};
}

void sgd_step(at::Tensor p, at::Tensor g, at::Tensor m, double lr, double mu,
              double wd, bool nesterov) {
  check_flat_state("sgd_step", p, {&g, &m});
  tfosr_sgd_step(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(),
                 (float)lr, (float)mu, (float)wd, nesterov, p.numel(),
                 cur_stream());
}

at::Tensor gemm_bt(at::Tensor a, at::Tensor b, bool out_bf16) {
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && a.size(1) == b.size(1),
              "gemm_bt: A[M,K], B[N,K]");
  TORCH_CHECK(a.scalar_type() == at::kBFloat16 && b.scalar_type() == at::kBFloat16);
  int M = a.size(0), N = b.size(0), K = a.size(1);
  if (K % 32 != 0) {
    int Kp = (K + 31) / 32 * 32;
    auto ap = at::zeros({M, Kp}, a.options());
    auto bp = at::zeros({N, Kp}, b.options());
    ap.narrow(1, 0, K).copy_(a);
    bp.narrow(1, 0, K).copy_(b);
    a = ap; b = bp; K = Kp;
  }
  a = a.contiguous();
  b = b.contiguous();
  auto out = at::empty({M, N}, a.options().dtype(out_bf16 ? at::kBFloat16
                                                          : at::kFloat));
  tfosr_gemm_bt(a.data_ptr(), b.data_ptr(), out.data_ptr(), out_bf16, M, N, K,
                cur_stream());
  return out;
}

// -> (c, part, rows_per_tile): c is gemm_bt(a, b, out_bf16=True) bit for bit;
// part[ceil(M / rows_per_tile)][2][N] are c's per-tile BatchNorm partials for
// bn_fwd_train_pre, or None (rows_per_tile 0) where the dispatched kernel has
// no statistics epilogue and the caller keeps the separate pass.
py::tuple gemm_bt_stats(at::Tensor a, at::Tensor b) {
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && a.size(1) == b.size(1),
              "gemm_bt_stats: A[M,K], B[N,K]");
  TORCH_CHECK(a.is_cuda(), "gemm_bt_stats: a must be a GPU tensor");
  TORCH_CHECK(b.device() == a.device(), "gemm_bt_stats: b must be on ",
              a.device());
  TORCH_CHECK(a.scalar_type() == at::kBFloat16 &&
                  b.scalar_type() == at::kBFloat16,
              "gemm_bt_stats: a and b must be bfloat16");
  const long M = a.size(0), N = b.size(0), K = a.size(1);
  TORCH_CHECK(M >= 1 && N >= 1 && K >= 1 && M <= INT_MAX && N <= INT_MAX &&
                  K <= INT_MAX, "gemm_bt_stats: bad sizes");
  const int rows = K % 32 == 0
      ? tfosr_gemm_bt_stats_rows((int)M, (int)N, (int)K) : 0;
  if (rows == 0)  // gemm_bt's own route (it also pads a ragged K)
    return py::make_tuple(gemm_bt(a, b, true), py::none(), 0);
  a = a.contiguous();
  b = b.contiguous();
  auto out = at::empty({M, N}, a.options());
  auto part = at::empty({(M + rows - 1) / rows, 2, N},
                        a.options().dtype(at::kFloat));
  tfosr_gemm_bt_stats(a.data_ptr(), b.data_ptr(), out.data_ptr(),
                      part.data_ptr<float>(), (int)M, (int)N, (int)K,
                      cur_stream());
  return py::make_tuple(out, part, rows);
}

at::Tensor gemm_bf16(at::Tensor a, at::Tensor b) {
  // A[M,K] @ B[K,N]: feed B^T (contiguous [N,K]) to the kernel
  return gemm_bt(a, b.t().contiguous(), /*out_bf16=*/false);
}

at::Tensor mfma_probe(at::Tensor a, at::Tensor b) {
  TORCH_CHECK(a.sizes() == at::IntArrayRef({64, 8}) &&
              b.sizes() == at::IntArrayRef({64, 8}));
  auto c = at::empty({64, 4}, a.options().dtype(at::kFloat));
  tfosr_mfma_probe(a.contiguous().data_ptr<short>(),
                   b.contiguous().data_ptr<short>(), c.data_ptr<float>(),
                   cur_stream());
  return c;
}

}  // namespace

// bump when the binding surface changes: the Python side refuses to run
// against a stale in-tree .so (clear "rebuild" message instead of a random
// AttributeError mid-training)
#define TFOSR_API_VERSION 8

// Largest filter reach fd*(k-1) the conv entries accept. The kernels form
// ih = oh*S - P + r*fd in int; image coordinates stay below 2^24 in any
// tensor that fits the device, so a reach capped at 2^20 keeps every such
// sum far inside the int range.
static constexpr long kMaxTapReach = 1L << 20;

// Which kernel a conv_mfma launch takes (csrc/conv3x3_halo.hip): the halo
// kernel covers the plain 3x3 stride-1 padding-1 bf16 launch of natural
// output size; TFOS_CONV3X3_TILE = auto | im2col | halo picks among the
// eligible ones, anything else is an error.
struct ConvTilePlan {
  bool halo;
  int bm, bn, max_w;
  long tiles, grid;
};

static ConvTilePlan conv3x3_tile_plan(long N, long H, long W, long Cin,
                                      long Cout, long fh, long fw, long S,
                                      long P, long D, long OH, long OW,
                                      long fd, bool out_f32, bool plain) {
  const bool eligible = plain && fh == 3 && fw == 3 && S == 1 && P == 1 &&
                        D == 1 && fd == 1 && !out_f32 && OH == H && OW == W;
  ConvTilePlan p;
  const int k = tfosr_conv3x3_halo_plan(eligible, (int)N, (int)H, (int)W,
                                        (int)Cin, (int)Cout, &p.bm, &p.bn,
                                        &p.tiles, &p.grid, &p.max_w);
  TORCH_CHECK(k != -1, "TFOS_CONV3X3_TILE must be auto, im2col or halo");
  TORCH_CHECK(k != -2, "TFOS_CONV3X3_HALO_BM must be 256 or 512");
  p.halo = k == 1;
  return p;
}

// conv_mfma and conv_mfma_stats (see their m.def below). stats: also return
// the output's BatchNorm tile partials [ceil(N*OH*OW / 256)][2][Cout] where
// the launch has the statistics epilogue (input dilation 1, bf16 output).
static std::pair<at::Tensor, c10::optional<at::Tensor>> conv_mfma_impl(
    at::Tensor x, at::Tensor wk, long Cout, long fh, long fw, long S, long P,
    long D, long OH, long OW, long fd, bool out_f32, bool stats) {
  TORCH_CHECK(x.dim() == 4 && x.is_contiguous(at::MemoryFormat::ChannelsLast),
              "conv_mfma expects channels_last input");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 &&
              wk.scalar_type() == at::kBFloat16);
  TORCH_CHECK(fh >= 1 && fw >= 1 && fh * fw <= 49, "bad filter dims");
  TORCH_CHECK(D == 1 || D == 2, "input dilation must be 1 or 2");
  TORCH_CHECK(fd >= 1, "conv_mfma: filter dilation fd must be >= 1, got ",
              fd);
  TORCH_CHECK(fd == 1 || D == 1,
              "conv_mfma: filter dilation fd > 1 requires input dilation "
              "D == 1");
  // ih = oh*S - P + r*fd is computed in int: keep the tap reach far
  // below 2^31 so it cannot overflow whatever the image size
  TORCH_CHECK(fd <= kMaxTapReach && fd * (fh - 1) <= kMaxTapReach &&
                  fd * (fw - 1) <= kMaxTapReach,
              "conv_mfma: fd, fd*(fh-1) and fd*(fw-1) must be <= ",
              kMaxTapReach);
  long taps = fh * fw;
  int N = x.size(0), Cin = x.size(1), H = x.size(2), W = x.size(3);
  TORCH_CHECK(Cin % 32 == 0, "conv_mfma requires Cin % 32 == 0");
  TORCH_CHECK(wk.size(1) == taps * Cin);
  if (OH < 0) {
    long HV = (H - 1) * D + 1, WV = (W - 1) * D + 1;
    long nh = HV + 2 * P - fd * (fh - 1) - 1;
    long nw = WV + 2 * P - fd * (fw - 1) - 1;
    TORCH_CHECK(nh >= 0 && nw >= 0,
                "conv_mfma: the dilated filter does not fit the padded "
                "input");
    OH = nh / S + 1;
    OW = nw / S + 1;
  }
  auto y = at::empty({N, Cout, OH, OW},
                     x.options().dtype(out_f32 ? at::kFloat : at::kBFloat16),
                     at::MemoryFormat::ChannelsLast);
  const void* guard = zero_guard(x);
  // before either launch, so that a bad TFOS_CONV3X3_TILE is an error on
  // every path; a launch with the statistics epilogue is never eligible
  const ConvTilePlan plan = conv3x3_tile_plan(N, H, W, Cin, Cout, fh, fw, S, P,
                                              D, OH, OW, fd, out_f32, !stats);
  if (stats && D == 1 && !out_f32) {
    TORCH_CHECK(x.is_cuda() && wk.device() == x.device(),
                "conv_mfma_stats: x and wk must be on one GPU");
    const long M = (long)N * OH * OW;
    auto part = at::empty({(M + 255) / 256, 2, Cout},
                          x.options().dtype(at::kFloat));
    tfosr_conv_mfma_stats(x.data_ptr(), wk.contiguous().data_ptr(),
                          guard, y.data_ptr(),
                          part.data_ptr<float>(), N, H, W, Cin, Cout, OH, OW, S,
                          P, taps, fw, (int)fd, cur_stream());
    return {y, part};
  }
  if (plan.halo) {
    TORCH_CHECK(x.is_cuda() && wk.device() == x.device(),
                "conv_mfma: x and wk must be on one GPU");
    tfosr_conv3x3_halo(x.data_ptr(), wk.contiguous().data_ptr(), y.data_ptr(),
                       plan.bm, N, H, W, Cin, (int)Cout, cur_stream());
    return {y, c10::nullopt};
  }
  tfosr_conv_mfma(x.data_ptr(), wk.contiguous().data_ptr(), guard,
                  y.data_ptr(), /*out_bf16=*/out_f32 ? 0 : 1, N, H, W, Cin,
                  Cout, OH, OW, S, P, taps, fw, D, 0, (int)fd, cur_stream());
  return {y, c10::nullopt};
}

// ---------------------------------------------------------------------------
// Depthwise 3x3 (csrc/dwconv3x3.hip): groups == C, padding 1, stride 1 or 2
// ---------------------------------------------------------------------------

static int dw_vec(const at::Tensor& t) {
  return t.scalar_type() == at::kBFloat16 ? 8 : 4;
}

// An activation or gradient as the kernels take it. Returns true when the
// tensor is empty (nothing to launch).
static bool dw_check_act(const char* op, const char* name,
                         const at::Tensor& t) {
  TORCH_CHECK(t.is_cuda(), op, ": ", name, " must be a GPU tensor");
  TORCH_CHECK(t.dim() == 4, op, ": ", name, " must be 4-D (N, C, H, W), got ",
              t.dim(), "-D");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16 ||
                  t.scalar_type() == at::kFloat,
              op, ": ", name, " must be bf16 or fp32, got ", t.scalar_type());
  if (t.numel() == 0) return true;
  TORCH_CHECK(t.is_contiguous(at::MemoryFormat::ChannelsLast), op, ": ", name,
              " must be channels_last-contiguous");
  const int V = dw_vec(t);
  TORCH_CHECK(t.size(1) % V == 0, op, ": C=", t.size(1),
              " must be a multiple of ", V, " for ", t.scalar_type());
  TORCH_CHECK((uintptr_t)t.data_ptr() % 16 == 0, op, ": ", name,
              " must be 16-byte aligned");
  TORCH_CHECK(t.numel() / V < (1L << 31), op, ": ", name, " has ", t.numel(),
              " elements, more than the kernels index");
  return false;
}

static void dw_check_weight(const char* op, const at::Tensor& w,
                            const at::Tensor& act) {
  TORCH_CHECK(w.device() == act.device(), op, ": weight must be on ",
              act.device(), ", got ", w.device());
  TORCH_CHECK(w.scalar_type() == at::kFloat && w.dim() == 4 &&
                  w.size(0) == act.size(1) && w.size(1) == 1 &&
                  w.size(2) == 3 && w.size(3) == 3 && w.is_contiguous(),
              op, ": weight must be the contiguous fp32 [C,1,3,3] parameter "
              "with C=", act.size(1), ", got ", w.scalar_type(), " ",
              w.sizes());
}

static void dw_check_stride(const char* op, long stride) {
  TORCH_CHECK(stride == 1 || stride == 2, op, ": stride must be 1 or 2, got ",
              stride);
}

static long dw_out(long in, long stride) { return (in - 1) / stride + 1; }

static at::Tensor dwconv3x3_fwd(at::Tensor x, at::Tensor w, long stride) {
  const char* op = "dwconv3x3_fwd";
  dw_check_stride(op, stride);
  const bool empty = dw_check_act(op, "x", x);
  dw_check_weight(op, w, x);
  const long N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const long OH = H > 0 ? dw_out(H, stride) : 0;
  const long OW = W > 0 ? dw_out(W, stride) : 0;
  auto y = at::empty({N, C, OH, OW}, x.options(),
                     at::MemoryFormat::ChannelsLast);
  if (empty) return y;
  tfosr_dwconv3x3_fwd(x.data_ptr(), w.data_ptr<float>(), y.data_ptr(),
                      x.scalar_type() == at::kBFloat16, N, C, H, W, OH, OW,
                      stride, cur_stream());
  return y;
}

static at::Tensor dwconv3x3_dgrad(at::Tensor dy, at::Tensor w, long stride,
                                  long H, long W) {
  const char* op = "dwconv3x3_dgrad";
  dw_check_stride(op, stride);
  const bool empty = dw_check_act(op, "dy", dy);
  dw_check_weight(op, w, dy);
  TORCH_CHECK(H >= 0 && W >= 0, op, ": H and W must not be negative");
  const long N = dy.size(0), C = dy.size(1);
  const long OH = H > 0 ? dw_out(H, stride) : 0;
  const long OW = W > 0 ? dw_out(W, stride) : 0;
  TORCH_CHECK(dy.size(2) == OH && dy.size(3) == OW, op, ": a ", H, "x", W,
              " input with stride ", stride, " gives ", OH, "x", OW,
              ", the gradient is ", dy.size(2), "x", dy.size(3));
  auto dx = at::empty({N, C, H, W}, dy.options(),
                      at::MemoryFormat::ChannelsLast);
  if (empty || dx.numel() == 0) return dx;
  TORCH_CHECK(dx.numel() / dw_vec(dy) < (1L << 31), op, ": dx has ",
              dx.numel(), " elements, more than the kernels index");
  tfosr_dwconv3x3_dgrad(dy.data_ptr(), w.data_ptr<float>(), dx.data_ptr(),
                        dy.scalar_type() == at::kBFloat16, N, C, H, W, OH, OW,
                        stride, cur_stream());
  return dx;
}

static at::Tensor dwconv3x3_wrw(at::Tensor dy, at::Tensor x, long stride) {
  const char* op = "dwconv3x3_wrw";
  dw_check_stride(op, stride);
  const bool dy_empty = dw_check_act(op, "dy", dy);
  const bool x_empty = dw_check_act(op, "x", x);
  TORCH_CHECK(x.device() == dy.device(), op, ": x must be on ", dy.device(),
              ", got ", x.device());
  TORCH_CHECK(x.scalar_type() == dy.scalar_type(), op,
              ": dy and x must have one dtype, got ", dy.scalar_type(),
              " and ", x.scalar_type());
  const long N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const long OH = H > 0 ? dw_out(H, stride) : 0;
  const long OW = W > 0 ? dw_out(W, stride) : 0;
  TORCH_CHECK(dy.size(0) == N && dy.size(1) == C && dy.size(2) == OH &&
                  dy.size(3) == OW,
              op, ": x ", x.sizes(), " with stride ", stride,
              " gives a gradient of [", N, ", ", C, ", ", OH, ", ", OW,
              "], got ", dy.sizes());
  auto opts = x.options().dtype(at::kFloat);
  if (dy_empty || x_empty) return at::zeros({C, 1, 3, 3}, opts);
  int grid_y, cvb, P, nblk;
  long slab;
  tfosr_dwconv3x3_wrw_plan(N * OH * OW, C / dw_vec(x), &grid_y, &cvb, &P,
                           &nblk, &slab);
  auto part = at::empty({(long)nblk, 9, C}, opts);
  auto dw = at::empty({C, 1, 3, 3}, opts);
  tfosr_dwconv3x3_wrw(dy.data_ptr(), x.data_ptr(), part.data_ptr<float>(),
                      dw.data_ptr<float>(), x.scalar_type() == at::kBFloat16,
                      N, C, H, W, OH, OW, stride, cur_stream());
  return dw;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("api_version", []() { return TFOSR_API_VERSION; });
  m.def("bn_fwd_train", &bn_fwd_train);
  m.def("bn_fwd_eval", &bn_fwd_eval);
  m.def("bn_bwd", &bn_bwd);
  m.def("bn_dual_eligible", &bn_dual_eligible);
  m.def("bn_dual_fwd_train", &bn_dual_fwd_train);
  m.def("bn_dual_bwd", &bn_dual_bwd);
  // blocks of the fast-path reduction kernels for a shape (0 = generic path):
  // tools/bn_bench.py counts the partials' bytes with it
  m.def("bn_fast_blocks", [](long total, int C, bool bf16, bool nhwc) {
    return tfosr_bn_fast_blocks(total, C, bf16, nhwc);
  });
  m.def("bn_stage", &bn_stage);
  m.def("softmax_xent_fwd", &softmax_xent_fwd);
  m.def("softmax_xent_bwd", &softmax_xent_bwd);
  m.def("xent_dense_fwd", &xent_dense_fwd, py::arg("logits"), py::arg("target"),
        py::arg("ignore_index") = -100, py::arg("label_smoothing") = 0.0,
        py::arg("reduction") = 0, py::arg("max_grid") = 0);
  m.def("xent_dense_bwd", &xent_dense_bwd, py::arg("logits"), py::arg("lse"),
        py::arg("target"), py::arg("gout"), py::arg("nvalid") = py::none(),
        py::arg("ignore_index") = -100, py::arg("label_smoothing") = 0.0,
        py::arg("reduction") = 0, py::arg("max_grid") = 0);
  m.def("nhwc_pack", &nhwc_pack);
  m.def("sgd_step", &sgd_step);
  m.def("adam_step", [](at::Tensor p, at::Tensor g, at::Tensor m, at::Tensor v,
                        double lr, double b1, double b2, double eps, double wd,
                        long step, bool decoupled) {
    check_flat_state("adam_step", p, {&g, &m, &v});
    TORCH_CHECK(step >= 1 && step <= INT_MAX,
                "adam_step: step counts from 1, got ", step);
    tfosr_adam_step(p.data_ptr<float>(), g.data_ptr<float>(),
                    m.data_ptr<float>(), v.data_ptr<float>(), lr, b1, b2, eps,
                    wd, (int)step, decoupled, p.numel(), cur_stream());
  });
  m.def("gemm_bt", &gemm_bt, py::arg("a"), py::arg("b"), py::arg("out_bf16") = false);
  m.def("gemm_bf16", &gemm_bf16);
  m.def("mfma_probe", &mfma_probe);
  m.def("maxpool_fwd", [](at::Tensor x, long K, long S, long P) {
    TORCH_CHECK(x.dim() == 4 && x.is_contiguous(at::MemoryFormat::ChannelsLast),
                "maxpool_fwd expects channels_last");
    auto ohw = check_pool_geometry("maxpool_fwd", x, x.size(1), x.size(0),
                                   x.size(2), x.size(3), K, S, P);
    int N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
    int OH = (int)ohw.first, OW = (int)ohw.second;
    auto y = at::empty({N, C, OH, OW}, x.options(),
                       at::MemoryFormat::ChannelsLast);
    auto idx = at::empty({N, OH, OW, C}, x.options().dtype(at::kByte));
    tfosr_maxpool_fwd(x.data_ptr(), y.data_ptr(), idx.data_ptr<unsigned char>(),
                      x.scalar_type() == at::kBFloat16, N, C, H, W, OH, OW,
                      K, S, P, cur_stream());
    return std::vector<at::Tensor>{y, idx};
  });
  m.def("conv3x3_fwd", [](at::Tensor x, at::Tensor w9, long Cout, long S,
                          long P) {
    TORCH_CHECK(x.dim() == 4 && x.is_contiguous(at::MemoryFormat::ChannelsLast),
                "conv3x3_fwd expects channels_last input");
    TORCH_CHECK(x.scalar_type() == at::kBFloat16 &&
                w9.scalar_type() == at::kBFloat16);
    int N = x.size(0), Cin = x.size(1), H = x.size(2), W = x.size(3);
    TORCH_CHECK(Cin % 32 == 0, "conv3x3 requires Cin % 32 == 0");
    TORCH_CHECK(w9.size(1) == 9 * Cin);
    int OH = (H + 2 * P - 3) / S + 1, OW = (W + 2 * P - 3) / S + 1;
    auto y = at::empty({N, Cout, OH, OW}, x.options(),
                       at::MemoryFormat::ChannelsLast);
    const void* guard = zero_guard(x);
    tfosr_conv3x3(x.data_ptr(), w9.contiguous().data_ptr(), guard,
                  y.data_ptr(), /*out_bf16=*/1, N, H, W, Cin, Cout, OH, OW,
                  S, P, cur_stream());
    return y;
  });
  // Generalized implicit-GEMM conv: taps in {1,9}, stride S, pad P, input
  // dilation D (the stored input is read as if zero-dilated by D). OH/OW are
  // explicit because backward-data output size is not derivable from the
  // stored input dims. One kernel covers conv1x1/conv3x3 fwd at stride 1/2,
  // their backward-data, and ConvTranspose2d k3 s2 (survey §2.3 rows 1-2).
  //
  // fd is the FILTER dilation (atrous conv): tap (r, s) reads the input at
  // offset (r*fd, s*fd), so the natural output size is
  // (H + 2P - fd*(fh-1) - 1)/S + 1. out_f32 returns the fp32 accumulator
  // unrounded instead of bf16.
  m.def("conv_mfma", [](at::Tensor x, at::Tensor wk, long Cout, long fh,
                        long fw, long S, long P, long D, long OH, long OW,
                        long fd, bool out_f32) {
    return conv_mfma_impl(x, wk, Cout, fh, fw, S, P, D, OH, OW, fd, out_f32,
                          /*stats=*/false).first;
  }, py::arg("x"), py::arg("wk"), py::arg("Cout"), py::arg("fh"),
     py::arg("fw"), py::arg("S"), py::arg("P"), py::arg("D"), py::arg("OH"),
     py::arg("OW"), py::arg("fd") = 1, py::arg("out_f32") = false);
  // Host only: the kernel conv_mfma would launch for this call under the
  // current TFOS_CONV3X3_TILE, with its tile, tile count and grid, and the
  // largest W the halo kernel can stage (OH/OW < 0: the natural size).
  m.def("conv3x3_halo_plan", [](long N, long H, long W, long Cin, long Cout,
                                long fh, long fw, long S, long P, long D,
                                long OH, long OW, long fd, bool out_f32) {
    TORCH_CHECK(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && S > 0 &&
                fd > 0 && D > 0, "conv3x3_halo_plan: bad dims");
    if (OH < 0) {
      OH = ((H - 1) * D + 1 + 2 * P - fd * (fh - 1) - 1) / S + 1;
      OW = ((W - 1) * D + 1 + 2 * P - fd * (fw - 1) - 1) / S + 1;
    }
    const ConvTilePlan p = conv3x3_tile_plan(N, H, W, Cin, Cout, fh, fw, S, P,
                                             D, OH, OW, fd, out_f32, true);
    py::dict d;
    d["kernel"] = p.halo ? "halo" : "im2col";
    d["BM"] = p.bm;
    d["BN"] = p.bn;
    d["tiles"] = p.tiles;
    d["grid"] = p.grid;
    d["max_w"] = p.max_w;
    return d;
  }, py::arg("N"), py::arg("H"), py::arg("W"), py::arg("Cin"),
     py::arg("Cout"), py::arg("fh") = 3, py::arg("fw") = 3, py::arg("S") = 1,
     py::arg("P") = 1, py::arg("D") = 1, py::arg("OH") = -1,
     py::arg("OW") = -1, py::arg("fd") = 1, py::arg("out_f32") = false);
  // -> (y, part, rows_per_tile): y is conv_mfma(...) bit for bit; part holds
  // y's per-tile BatchNorm partials for bn_fwd_train_pre, or None
  // (rows_per_tile 0) where the launch has no statistics epilogue (input
  // dilation 2 or fp32 output) and the caller keeps the separate pass.
  m.def("conv_mfma_stats", [](at::Tensor x, at::Tensor wk, long Cout, long fh,
                              long fw, long S, long P, long D, long OH,
                              long OW, long fd, bool out_f32) {
    auto r = conv_mfma_impl(x, wk, Cout, fh, fw, S, P, D, OH, OW, fd, out_f32,
                            /*stats=*/true);
    if (!r.second.has_value()) return py::make_tuple(r.first, py::none(), 0);
    return py::make_tuple(r.first, *r.second, 256);
  }, py::arg("x"), py::arg("wk"), py::arg("Cout"), py::arg("fh"),
     py::arg("fw"), py::arg("S"), py::arg("P"), py::arg("D"), py::arg("OH"),
     py::arg("OW"), py::arg("fd") = 1, py::arg("out_f32") = false);
  m.def("gemm_bt_stats", &gemm_bt_stats, py::arg("a"), py::arg("b"));
  m.def("bn_fwd_train_pre", &bn_fwd_train_pre);
  m.def("bn_dual_fwd_train_pre", &bn_dual_fwd_train_pre);
  m.def("bn_batch_stats", &bn_batch_stats);
  // conv_mfma accumulating INTO an existing channels_last tensor:
  // out += conv(x, wk) — fuses the residual-join gradient accumulation the
  // eager autograd would do as a separate whole-tensor add (8.4 ms/step of
  // CUDAFunctor_add at ResNet-50 b1024, profiles/README r01).
  m.def("conv_mfma_acc", [](at::Tensor x, at::Tensor wk, at::Tensor out,
                            long fh, long fw, long S, long P, long D) {
    TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast) &&
                out.is_contiguous(at::MemoryFormat::ChannelsLast));
    TORCH_CHECK(x.scalar_type() == at::kBFloat16 &&
                wk.scalar_type() == at::kBFloat16 &&
                out.scalar_type() == at::kBFloat16);
    int N = x.size(0), Cin = x.size(1), H = x.size(2), W = x.size(3);
    TORCH_CHECK(Cin % 32 == 0, "conv_mfma requires Cin % 32 == 0");
    long taps = fh * fw;
    TORCH_CHECK(wk.size(1) == taps * Cin);
    long Cout = out.size(1), OH = out.size(2), OW = out.size(3);
    TORCH_CHECK(out.size(0) == N);
    const void* guard = zero_guard(x);
    tfosr_conv_mfma(x.data_ptr(), wk.contiguous().data_ptr(), guard,
                    out.data_ptr(), /*out_bf16=*/1, N, H, W, Cin, Cout, OH, OW,
                    S, P, taps, fw, D, 1, /*fd=*/1, cur_stream());
    return out;
  });
  // gemm accumulating into an existing [M, N] tensor: C += A @ B^T.
  // bf16 only: the launcher instantiates the accumulating epilogue for bf16
  // output alone, so an fp32 c would be overwritten instead of added to.
  m.def("gemm_bt_acc", [](at::Tensor a, at::Tensor b, at::Tensor c) {
    TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && c.dim() == 2,
                "gemm_bt_acc: A[M,K], B[N,K], C[M,N] must be 2-D");
    TORCH_CHECK(a.is_cuda(), "gemm_bt_acc: a must be a GPU tensor");
    TORCH_CHECK(b.device() == a.device() && c.device() == a.device(),
                "gemm_bt_acc: b and c must be on ", a.device());
    TORCH_CHECK(a.is_contiguous() && b.is_contiguous() && c.is_contiguous(),
                "gemm_bt_acc: a, b and c must be contiguous");
    TORCH_CHECK(a.scalar_type() == at::kBFloat16 &&
                    b.scalar_type() == at::kBFloat16 &&
                    c.scalar_type() == at::kBFloat16,
                "gemm_bt_acc: a, b and c must be bfloat16");
    long M = a.size(0), K = a.size(1), Nn = b.size(0);
    TORCH_CHECK(b.size(1) == K && c.size(0) == M && c.size(1) == Nn,
                "gemm_bt_acc: A[M,K], B[N,K], C[M,N]");
    TORCH_CHECK(K % 32 == 0, "gemm_bt_acc: K must be a multiple of 32");
    tfosr_gemm_bt_acc(a.data_ptr(), b.data_ptr(), c.data_ptr(),
                      /*out_bf16=*/1, M, Nn, K, 1, cur_stream());
    return c;
  });
  // wrw v2: MFMA + hardware transpose-reads + split-M workspace.
  // dy [N,Cout,OH,OW] cl, x [N,Cin,H,W] cl; filter R x S_f, conv stride,
  // pad P. Returns fp32 dW [Cout, R*S_f*Cin].
  // fd: filter dilation of the 3x3 case (dW tap (r, s) pairs dy[oh, ow]
  // with x[oh*stride - P + r*fd, ow*stride - P + s*fd]).
  m.def("conv_wrw2", [](at::Tensor dy, at::Tensor x, long R, long S_f,
                        long stride, long P, long fd) {
    TORCH_CHECK(dy.is_contiguous(at::MemoryFormat::ChannelsLast) &&
                x.is_contiguous(at::MemoryFormat::ChannelsLast));
    TORCH_CHECK(dy.scalar_type() == at::kBFloat16 &&
                x.scalar_type() == at::kBFloat16);
    int N = x.size(0), Cin = x.size(1), H = x.size(2), W = x.size(3);
    int Cout = dy.size(1), OH = dy.size(2), OW = dy.size(3);
    TORCH_CHECK(Cin % 8 == 0 && Cout % 8 == 0,
                "conv_wrw2 needs channel counts % 8 == 0");
    long taps = R * S_f;
    TORCH_CHECK(taps == 1 || taps == 9, "conv_wrw2 supports 1x1 and 3x3");
    TORCH_CHECK(fd >= 1, "conv_wrw2: filter dilation fd must be >= 1, got ",
                fd);
    TORCH_CHECK(taps != 1 || fd == 1,
                "conv_wrw2: a 1x1 filter has no dilation, fd must be 1");
    TORCH_CHECK(fd <= kMaxTapReach && fd * (R - 1) <= kMaxTapReach &&
                    fd * (S_f - 1) <= kMaxTapReach,
                "conv_wrw2: fd, fd*(R-1) and fd*(S_f-1) must be <= ",
                kMaxTapReach);
    long M = (long)N * OH * OW;
    int split = tfosr_wrw2_split(Cout, Cin, M);
    long K = taps * (long)Cin;
    // the split reduce indexes the workspace with 32-bit offsets
    TORCH_CHECK((long)split * Cout * K < (1L << 32),
                "conv_wrw2: the split workspace exceeds 2^32 elements");
    auto ws = at::empty({(long)split, (long)Cout * K},
                        x.options().dtype(at::kFloat));
    auto dW = at::empty({(long)Cout, K}, x.options().dtype(at::kFloat));
    const void* guard = zero_guard(x);
    tfosr_conv_wrw2(dy.data_ptr(), x.data_ptr(), guard,
                    ws.data_ptr<float>(), dW.data_ptr<float>(), N, H, W, Cin,
                    Cout, OH, OW, R, S_f, stride, P, split, (int)fd,
                    cur_stream());
    return dW;
  }, py::arg("dy"), py::arg("x"), py::arg("R"), py::arg("S_f"),
     py::arg("stride"), py::arg("P"), py::arg("fd") = 1);
  // One parity class of a stride-2 backward-data / transposed conv:
  // out[oh*2+oh0, ow*2+ow0] = conv(x, wk_class) with the class's taps
  // (list of (r,s) pairs). wk_class: [Cout, ntaps*Cin]. Writes into `out`
  // (pre-allocated [N, Cout, OHr, OWr] channels_last; classes disjoint).
  // batched weight pack: desc buffer layout must match PackDesc in
  // elementwise.hip (built by ops/packplan.py); one launch packs every
  // per-step weight transform into the bf16 arena
  m.def("pack_bf16", [](at::Tensor descs, at::Tensor cum, long ndesc,
                        at::Tensor arena, long total) {
    TORCH_CHECK(descs.is_cuda() && cum.is_cuda() && arena.is_cuda() &&
                    descs.device() == arena.device() &&
                    cum.device() == arena.device(),
                "pack_bf16 expects descs, cum and arena on one GPU");
    TORCH_CHECK(arena.scalar_type() == at::kBFloat16 && arena.is_contiguous(),
                "pack_bf16 expects a contiguous bf16 arena");
    TORCH_CHECK(ndesc >= 0 && ndesc <= INT_MAX, "pack_bf16: bad ndesc ", ndesc);
    // 80 bytes = sizeof(PackDesc) in elementwise.hip
    TORCH_CHECK(descs.scalar_type() == at::kByte && descs.is_contiguous() &&
                    descs.numel() == ndesc * 80,
                "pack_bf16: descs must hold ndesc * 80 contiguous bytes");
    TORCH_CHECK(cum.scalar_type() == at::kLong && cum.is_contiguous() &&
                    cum.numel() == ndesc + 1,
                "pack_bf16: cum must hold ndesc + 1 contiguous int64");
    TORCH_CHECK(total >= 0 && arena.numel() >= total,
                "pack_bf16: arena holds ", arena.numel(), " elements, total is ",
                total);
    if (total == 0) return;
    TORCH_CHECK(ndesc >= 1, "pack_bf16: no descriptor for ", total, " elements");
    tfosr_pack_bf16(descs.data_ptr(), cum.data_ptr(), (int)ndesc,
                    arena.data_ptr(), total, cur_stream());
  });
  m.def("conv_par", [](at::Tensor x, at::Tensor wk, at::Tensor out,
                       std::vector<long> taps_r, std::vector<long> taps_s,
                       long P, bool accum) {
    TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast) &&
                out.is_contiguous(at::MemoryFormat::ChannelsLast));
    TORCH_CHECK(x.scalar_type() == at::kBFloat16 &&
                wk.scalar_type() == at::kBFloat16 &&
                out.scalar_type() == at::kBFloat16);
    int N = x.size(0), Cin = x.size(1), H = x.size(2), W = x.size(3);
    TORCH_CHECK(Cin % 32 == 0);
    long ntaps = (long)taps_r.size();
    TORCH_CHECK(ntaps >= 1 && ntaps <= 8 && taps_s.size() == (size_t)ntaps);
    TORCH_CHECK(wk.size(1) == ntaps * Cin);
    long Cout = out.size(1), OHr = out.size(2), OWr = out.size(3);
    // parity offsets come from the tap list: ihv = (oh*2+oh0) - P + r must be
    // even for every class tap — caller passes oh0/ow0 via taps parity
    // (we derive them from the first tap)
    long oh0 = ((P - taps_r[0]) % 2 + 2) % 2;
    long ow0 = ((P - taps_s[0]) % 2 + 2) % 2;
    long OHs = (OHr - oh0 + 1) / 2, OWs = (OWr - ow0 + 1) / 2;
    if (OHs <= 0 || OWs <= 0) return out;
    unsigned long pack = 0;
    for (long i = 0; i < ntaps; ++i)
      pack |= ((unsigned long)((taps_r[i] << 4) | taps_s[i])) << (i * 8);
    const void* guard = zero_guard(x);
    tfosr_conv_par(x.data_ptr(), wk.contiguous().data_ptr(), guard,
                   out.data_ptr(), N, H, W, Cin, (int)Cout, (int)OHs,
                   (int)OWs, (int)P, (int)ntaps, pack, (int)oh0, (int)ow0,
                   (int)OWr, OHr * OWr, accum ? 1 : 0, cur_stream());
    return out;
  });
  // ResNet stem: 7x7/s2/p3 conv over a pre-padded NHWC4 image
  // ([N,4,230,230] channels_last bf16, Cin 3->4 zero-padded, spatial pad 3
  // baked in); weight pre-packed to [Cout, 7*32] with zero columns for the
  // pads. Output [N, Cout, 112, 112].
  m.def("conv_stem", [](at::Tensor x4, at::Tensor w224, long Cout) {
    TORCH_CHECK(x4.is_contiguous(at::MemoryFormat::ChannelsLast) &&
                x4.size(1) == 4, "conv_stem expects NHWC4 padded input");
    TORCH_CHECK(x4.scalar_type() == at::kBFloat16 &&
                w224.scalar_type() == at::kBFloat16);
    TORCH_CHECK(w224.size(1) == 224);
    int N = x4.size(0), Hp = x4.size(2), Wp = x4.size(3);
    int OH = (Hp - 7) / 2 + 1, OW = (Wp - 7) / 2 + 1;
    auto y = at::empty({N, Cout, OH, OW}, x4.options(),
                       at::MemoryFormat::ChannelsLast);
    const void* guard = zero_guard(x4);
    tfosr_conv_stem(x4.data_ptr(), w224.contiguous().data_ptr(),
                    guard, y.data_ptr(), N, Hp, Wp, Cout, OH, OW,
                    cur_stream());
    return y;
  });
  // stem weight gradient over the same NHWC4 padded view: returns fp32
  // [Cout, 7*32] (rows x (8 px x 4 ch), pads included — caller unpacks)
  m.def("conv_stem_wrw", [](at::Tensor dy, at::Tensor x4) {
    TORCH_CHECK(dy.is_contiguous(at::MemoryFormat::ChannelsLast) &&
                x4.is_contiguous(at::MemoryFormat::ChannelsLast));
    TORCH_CHECK(dy.scalar_type() == at::kBFloat16 &&
                x4.scalar_type() == at::kBFloat16 && x4.size(1) == 4);
    int N = x4.size(0), Hp = x4.size(2), Wp = x4.size(3);
    int Cout = dy.size(1), OH = dy.size(2), OW = dy.size(3);
    long M = (long)N * OH * OW;
    int split = tfosr_wrw2_split(Cout, 32, M);
    long K = 7L * 32;
    TORCH_CHECK((long)split * Cout * K < (1L << 32),
                "conv_stem_wrw: the split workspace exceeds 2^32 elements");
    auto ws = at::empty({(long)split, (long)Cout * K},
                        x4.options().dtype(at::kFloat));
    auto dW = at::empty({(long)Cout, K}, x4.options().dtype(at::kFloat));
    const void* guard = zero_guard(x4);
    tfosr_conv_wrw2(dy.data_ptr(), x4.data_ptr(), guard,
                    ws.data_ptr<float>(), dW.data_ptr<float>(), N, Hp, Wp,
                    /*Cin=*/32, Cout, OH, OW, /*R=*/7, /*S_f=*/1,
                    /*stride=*/2, /*P=*/0, split, /*fd=*/1, cur_stream());
    return dW;
  });
  m.def("conv_wrw", [](at::Tensor dy, at::Tensor x, long R, long S, long P) {
    TORCH_CHECK(dy.is_contiguous(at::MemoryFormat::ChannelsLast) &&
                x.is_contiguous(at::MemoryFormat::ChannelsLast));
    TORCH_CHECK(dy.scalar_type() == at::kBFloat16 &&
                x.scalar_type() == at::kBFloat16);
    int N = x.size(0), Cin = x.size(1), H = x.size(2), W = x.size(3);
    int Cout = dy.size(1), OH = dy.size(2), OW = dy.size(3);
    auto dW = at::zeros({Cout, R * S * (long)Cin},
                        x.options().dtype(at::kFloat));
    tfosr_conv_wrw(dy.data_ptr(), x.data_ptr(), dW.data_ptr<float>(), N, H, W,
                   Cin, Cout, OH, OW, R, S, P, cur_stream());
    return dW;
  });
  m.def("maxpool_bwd", [](at::Tensor dy, at::Tensor idx, long H, long W,
                          long K, long S, long P) {
    TORCH_CHECK(dy.dim() == 4, "maxpool_bwd expects a 4-D gradient");
    auto ohw = check_pool_geometry("maxpool_bwd", dy, dy.size(1), dy.size(0),
                                   H, W, K, S, P);
    TORCH_CHECK(dy.size(2) == ohw.first && dy.size(3) == ohw.second,
                "maxpool_bwd: a ", H, "x", W, " input pooled with K=", K,
                " S=", S, " P=", P, " gives ", ohw.first, "x", ohw.second,
                ", the gradient is ", dy.size(2), "x", dy.size(3));
    TORCH_CHECK(idx.scalar_type() == at::kByte && idx.is_contiguous() &&
                    idx.device() == dy.device() && idx.dim() == 4 &&
                    idx.size(0) == dy.size(0) && idx.size(1) == dy.size(2) &&
                    idx.size(2) == dy.size(3) && idx.size(3) == dy.size(1),
                "maxpool_bwd: idx must be the contiguous uint8 (N, OH, OW, C) "
                "tensor maxpool_fwd returned, on the gradient's device");
    dy = dy.contiguous(at::MemoryFormat::ChannelsLast);
    int N = dy.size(0), C = dy.size(1), OH = dy.size(2), OW = dy.size(3);
    auto dx = at::empty({N, C, H, W}, dy.options(),
                        at::MemoryFormat::ChannelsLast);
    tfosr_maxpool_bwd(dy.data_ptr(), idx.data_ptr<unsigned char>(),
                      dx.data_ptr(), dy.scalar_type() == at::kBFloat16,
                      N, C, H, W, OH, OW, K, S, P, cur_stream());
    return dx;
  });
  m.def("dwconv3x3_fwd", &dwconv3x3_fwd, py::arg("x"), py::arg("w"),
        py::arg("stride"));
  m.def("dwconv3x3_dgrad", &dwconv3x3_dgrad, py::arg("dy"), py::arg("w"),
        py::arg("stride"), py::arg("H"), py::arg("W"));
  m.def("dwconv3x3_wrw", &dwconv3x3_wrw, py::arg("dy"), py::arg("x"),
        py::arg("stride"));
  // launch constants and the wrw split, for sizing tests and benchmarks
  m.def("dwconv3x3_info", []() {
    int block, max_grid, strip, pair, min_pix, max_blocks, fin_lanes;
    tfosr_dwconv3x3_info(&block, &max_grid, &strip, &pair, &min_pix,
                         &max_blocks, &fin_lanes);
    py::dict d;
    d["block"] = block;
    d["max_grid"] = max_grid;
    d["strip"] = strip;
    d["pair"] = pair;
    d["wrw_min_pix"] = min_pix;
    d["wrw_max_blocks"] = max_blocks;
    d["fin_lanes"] = fin_lanes;
    return d;
  });
  m.def("dwconv3x3_wrw_plan", [](long M, long Cv) {
    TORCH_CHECK(M > 0 && Cv > 0, "dwconv3x3_wrw_plan: M and Cv must be "
                "positive");
    int grid_y, cvb, P, nblk;
    long slab;
    tfosr_dwconv3x3_wrw_plan(M, (int)Cv, &grid_y, &cvb, &P, &nblk, &slab);
    py::dict d;
    d["grid_y"] = grid_y;
    d["cvb"] = cvb;
    d["P"] = P;
    d["nblk"] = nblk;
    d["slab"] = slab;
    return d;
  });

  // native TFRecord codec (CPU): bulk scan/write with HW CRC32-C
  m.def("crc32c", [](py::bytes data) {
    std::string s = data;
    return tfosr::crc32c((const uint8_t*)s.data(), s.size(), 0);
  });
  m.def("tfrecord_read_file", [](const std::string& path, bool verify) {
    auto res = tfosr::scan_file(path, verify);
    py::list out;
    for (auto& [off, len] : res.records)
      out.append(py::bytes(res.buffer.data() + off, len));
    return out;
  }, py::arg("path"), py::arg("verify") = false);
  m.def("tfrecord_write_file",
        [](const std::string& path, const std::vector<std::string>& recs,
           bool append) { tfosr::write_file(path, recs, append); },
        py::arg("path"), py::arg("records"), py::arg("append") = false);
}
