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
int tfosr_bn_rows_mode();
int tfosr_bn_rows_plan(long, int, int, int, int*, int*);
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
int tfosr_gemm_bt_gate_eligible(int, int, int);
void tfosr_gemm_bt_gate(const void*, const void*, const void*,
                        const unsigned char*, void*, int, int, int,
                        hipStream_t);
void tfosr_mfma_probe(const short*, const short*, float*, hipStream_t);
void tfosr_maxpool_fwd(const void*, void*, unsigned char*, int, int, int, int,
                       int, int, int, int, int, int, hipStream_t);
void tfosr_maxpool_bwd(const void*, const unsigned char*, void*, int, int, int,
                       int, int, int, int, int, int, int, hipStream_t);
int tfosr_bn_pool_eligible(long, long, long, long, long);
int tfosr_bn_pool_blocks(long);
void tfosr_bn_relu_pool_fwd(const void*, void*, unsigned char*, const float*,
                            const float*, const float*, const float*, int, int,
                            int, int, int, int, int, int, int, hipStream_t);
void tfosr_bn_relu_pool_bwd_stats(const void*, const void*,
                                  const unsigned char*, const float*,
                                  const float*, float*, int, int, int, int, int,
                                  int, int, int, int, int, hipStream_t);
void tfosr_bn_relu_pool_bwd_dx(const void*, const void*, const unsigned char*,
                               void*, const float*, const float*, const float*,
                               const float*, const float*, int, int, int, int,
                               int, int, int, int, int, hipStream_t);
void tfosr_dwconv3x3_info(int*, int*, int*, int*, int*, int*, int*);
void tfosr_dwconv3x3_wrw_plan(long, int, int*, int*, int*, int*, long*);
void tfosr_dwconv3x3_fwd(const void*, const float*, void*, int, int, int, int,
                         int, int, int, int, hipStream_t);
void tfosr_dwconv3x3_dgrad(const void*, const float*, void*, int, int, int, int,
                           int, int, int, int, hipStream_t);
void tfosr_dwconv3x3_wrw(const void*, const void*, float*, float*, int, int,
                         int, int, int, int, int, int, hipStream_t);
void tfosr_convt_head_info(int*, int*, int*, int*, int*, int*, int*, int*, int*,
                           int*);
void tfosr_convt_head_wrw_plan(long, int, int, int*, long*);
void tfosr_convt_head_fwd(const void*, const float*, const float*, void*, int,
                          int, int, int, int, hipStream_t);
void tfosr_convt_head_dgrad(const void*, const float*, void*, int, int, int,
                            int, int, hipStream_t);
void tfosr_convt_head_wrw(const void*, const void*, float*, float*, float*,
                          int, int, int, int, int, hipStream_t);
int tfosr_convt_wrw_plan(long, int, int, int, int, int*, int*, int*, int*, int*,
                         long*, int*);
hipError_t tfosr_convt_wrw(const void*, const void*, float*, float*, long, int,
                           int, int, int, long, long, hipStream_t);
void tfosr_pwconv_info(int*, int*, int*);
void tfosr_pwconv_plan(long, int, int, int*, long*, int*, int*, int*, int*);
hipError_t tfosr_pwconv_gemm(const void*, const void*, int, void*, long, int,
                             int, int, hipStream_t);
void tfosr_upsample_bilinear_info(int*, int*, int*, int*, int*, int*, int*,
                                  int*, int*);
void tfosr_upsample_bilinear_plan(int, int, int, int, int, int, int, int*,
                                  int*, int*, long*, int*, int*, long*);
void tfosr_upsample_bilinear_fwd(const void*, void*, int, int, int, int, int,
                                 int, int, int, hipStream_t);
void tfosr_upsample_bilinear_bwd(const void*, void*, int, int, int, int, int,
                                 int, int, int, hipStream_t);
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

// Which tier of csrc/bn_relu.hip a tensor takes and the rows of partials its
// reductions write: the NHWC fast path, the NHWC row tier (TFOS_BN_ROWS = on,
// the default, or off; read at every call, anything else is an error) or,
// with nb == 0, the generic kernels, which add into a ZEROED [2C] workspace.
// Only the fast path writes and reads the ReLU bitmask.
struct BNTier {
  int nb;
  bool fast;
  int pixel_lanes, threads;  // of the row tier, else 0
};

static BNTier bn_tier(long total, int C, int bf, int nhwc) {
  TORCH_CHECK(tfosr_bn_rows_mode() >= 0, "TFOS_BN_ROWS must be on or off");
  BNTier t = {tfosr_bn_fast_blocks(total, C, bf, nhwc), true, 0, 0};
  if (t.nb > 0) return t;
  t.fast = false;
  t.nb = tfosr_bn_rows_plan(total, C, bf, nhwc, &t.pixel_lanes, &t.threads);
  return t;
}

static at::Tensor bn_workspace(const BNTier& t, int C,
                               const at::TensorOptions& opts) {
  return t.nb > 0 ? at::empty({(long)t.nb * 2 * C}, opts)
                  : at::zeros({2L * C}, opts);
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
  const BNTier tier = bn_tier(M * l.C, l.C, bf, l.nhwc);
  const int nb = tier.nb;
  auto ws = bn_workspace(tier, l.C, opts);
  auto save_mean = at::empty({l.C}, opts);
  auto save_rstd = at::empty({l.C}, opts);
  auto y = at::empty_like(x);
  // relu sign bitmask (1 byte per vector) for y-free backward gating
  at::Tensor mask;
  unsigned char* mask_ptr = nullptr;
  if (relu && tier.fast) {
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
  TORCH_CHECK(tfosr_bn_rows_mode() >= 0, "TFOS_BN_ROWS must be on or off");
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
  const BNTier tier = bn_tier(total, l.C, bf, l.nhwc);
  const int nb = tier.nb;
  auto ws = bn_workspace(tier, l.C, opts);
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
  TORCH_CHECK(!(relu && tier.fast) || mask_ptr != nullptr,
              "fast-path relu backward requires the forward bitmask");
  if (relu && tier.fast) {
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

// One launch of one BatchNorm kernel family on caller-owned tensors, in the
// tier bn_fwd_train / bn_bwd would take for x (fast path, row tier, generic), so
// that tools/bn_bench.py can time stats, apply, bwd stats and bwd dx apart
// (bn_fwd_train / bn_bwd run three launches each). family: 0 stats (x -> ws),
// 1 apply (x, other = res or none -> out, mask), 2 bwd stats (x, other = dy,
// mask -> ws, out = gout or none), 3 bwd dx (x, other = dy, mask -> out).
// p0..p3 are per-channel fp32 vectors: mean, rstd, weight, bias for apply;
// mean, rstd for bwd stats; mean, rstd, weight, dgamma for bwd dx with
// dbeta in p4. ws holds max(nb, 1) * 2C floats, nb = bn_fast_blocks() or else
// bn_rows_plan()[0]; the generic kernels (nb == 0) add into it, so the sums
// mean something only if the caller zeroed it. Off the fast path the mask is
// not used and a ReLU backward gates on y, which it then needs.
void bn_stage(int family, at::Tensor x, c10::optional<at::Tensor> other,
              c10::optional<at::Tensor> out, c10::optional<at::Tensor> mask,
              at::Tensor ws, std::vector<at::Tensor> p, bool relu,
              c10::optional<at::Tensor> y) {
  auto l = bn_layout(x);
  int bf = dtype_flag(x);
  long total = (long)l.N * l.HW * l.C;
  const BNTier tier = bn_tier(total, l.C, bf, l.nhwc);
  const int nb = tier.nb;
  TORCH_CHECK(l.nhwc, "bn_stage: expects a channels_last tensor");
  const size_t need[4] = {0, 4, 2, 5};
  TORCH_CHECK(family >= 0 && family < 4, "bn_stage: family must be 0..3");
  TORCH_CHECK(p.size() == need[family], "bn_stage: family ", family, " takes ",
              need[family], " per-channel vectors");
  for (auto& t : p) bn_check_channel_vec(t, x, l.C, "per-channel vector");
  TORCH_CHECK(ws.device() == x.device() && ws.scalar_type() == at::kFloat &&
                  ws.is_contiguous() &&
                  ws.numel() >= (long)(nb > 0 ? nb : 1) * 2 * l.C,
              "bn_stage: ws must hold max(nb, 1) * 2C floats");
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
  const void* y_ptr = nullptr;
  if (y.has_value()) {
    bn_check_like(*y, x, l.nhwc, true, "y");
    y_ptr = y->data_ptr();
  }
  if (family >= 2)
    TORCH_CHECK(!relu || (tier.fast ? (const void*)mask_ptr : y_ptr) != nullptr,
                "bn_stage: relu needs the mask on the fast path, y elsewhere");
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
      tfosr_bn_bwd_stats(x.data_ptr(), other_ptr, y_ptr, mask_ptr, out_ptr,
                         f(0), f(1), ws.data_ptr<float>(), nb, bf, 1, relu,
                         l.N, l.C, l.HW, s);
      break;
    default:
      tfosr_bn_bwd_dx(x.data_ptr(), other_ptr, y_ptr, mask_ptr, f(0), f(1),
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

// BatchNorm + ReLU + MaxPool2d as one op (csrc/bn_pool.hip): the ResNet stem's
// tail in training, on bf16 channels_last tensors the NHWC fast path of
// bn_relu.hip takes. bn_relu_pool_eligible() says whether the fused entries
// take a tensor and never throws; callers run bn_fwd_train + maxpool_fwd
// otherwise.
bool bn_relu_pool_eligible(const at::Tensor& x, long K, long S, long P) {
  if (!x.is_cuda() || x.dim() != 4 || x.scalar_type() != at::kBFloat16 ||
      !x.is_contiguous(at::MemoryFormat::ChannelsLast))
    return false;
  const long N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  if (N < 1 || H < 1 || W < 1 || K < 1 || S < 1 || P < 0 || P > K / 2 ||
      H + 2 * P < K || W + 2 * P < K || S > INT_MAX)
    return false;
  return tfosr_bn_pool_eligible(N, C, H, W, K) != 0;
}

// the checks both fused entries share; returns {OH, OW}
static std::pair<long, long> bn_relu_pool_check(const char* op,
                                                const at::Tensor& x, long K,
                                                long S, long P) {
  auto l = bn_layout(x);
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && l.nhwc, op,
              " expects a bf16 channels_last GPU tensor");
  auto ohw = check_pool_geometry(op, x, l.C, l.N, x.size(2), x.size(3), K, S, P);
  TORCH_CHECK(bn_relu_pool_eligible(x, K, S, P), op,
              ": needs N >= 1, C a multiple of 8 that divides 2048, fewer than "
              "2^31 elements and K*K <= 255; got shape ", x.sizes(), ", K=", K);
  return ohw;
}

// -> (p, idx, save_mean, save_rstd). The statistics are those of bn_fwd_train
// (same pass over x, same finalize, which updates the running statistics);
// p = maxpool(relu(bn(x))) and idx its (N, OH, OW, C) uint8 tap index, 0xFF
// where the window's maximum is not positive.
std::vector<at::Tensor> bn_relu_pool_fwd(at::Tensor x, at::Tensor w,
                                         at::Tensor b, at::Tensor rm,
                                         at::Tensor rv, double momentum,
                                         double eps, long K, long S, long P) {
  auto ohw = bn_relu_pool_check("bn_relu_pool_fwd", x, K, S, P);
  const int N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int OH = (int)ohw.first, OW = (int)ohw.second;
  bn_check_channel_vec(w, x, C, "weight");
  bn_check_channel_vec(b, x, C, "bias");
  bn_check_channel_vec(rm, x, C, "running_mean");
  bn_check_channel_vec(rv, x, C, "running_var");
  auto opts = x.options().dtype(at::kFloat);
  const long HW = (long)H * W, M = (long)N * HW;
  const BNTier tier = bn_tier(M * C, C, 1, 1);
  TORCH_CHECK(tier.fast, "bn_relu_pool_fwd: not a fast-path shape");
  auto ws = bn_workspace(tier, C, opts);
  auto save_mean = at::empty({C}, opts);
  auto save_rstd = at::empty({C}, opts);
  auto p = at::empty({N, C, OH, OW}, x.options(), at::MemoryFormat::ChannelsLast);
  auto idx = at::empty({N, OH, OW, C}, x.options().dtype(at::kByte));
  auto s = cur_stream();
  tfosr_bn_stats(x.data_ptr(), 1, 1, ws.data_ptr<float>(), tier.nb, N, C, HW, s);
  tfosr_bn_finalize(ws.data_ptr<float>(), tier.nb, x.data_ptr(), 1, 1, HW,
                    save_mean.data_ptr<float>(), save_rstd.data_ptr<float>(),
                    rm.data_ptr<float>(), rv.data_ptr<float>(), M, C,
                    (float)momentum, (float)eps, s);
  tfosr_bn_relu_pool_fwd(x.data_ptr(), p.data_ptr(),
                         idx.data_ptr<unsigned char>(),
                         save_mean.data_ptr<float>(),
                         save_rstd.data_ptr<float>(), w.data_ptr<float>(),
                         b.data_ptr<float>(), N, C, H, W, OH, OW, (int)K,
                         (int)S, (int)P, s);
  return {p, idx, save_mean, save_rstd};
}

// -> (dx, dgamma, dbeta) from the conv output x, the pooled gradient dp and
// the idx bn_relu_pool_fwd returned
std::vector<at::Tensor> bn_relu_pool_bwd(at::Tensor x, at::Tensor dp,
                                         at::Tensor idx, at::Tensor w,
                                         at::Tensor save_mean,
                                         at::Tensor save_rstd, long K, long S,
                                         long P) {
  auto ohw = bn_relu_pool_check("bn_relu_pool_bwd", x, K, S, P);
  const int N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int OH = (int)ohw.first, OW = (int)ohw.second;
  TORCH_CHECK(dp.device() == x.device() && dp.scalar_type() == at::kBFloat16 &&
                  dp.dim() == 4 && dp.size(0) == N && dp.size(1) == C &&
                  dp.size(2) == OH && dp.size(3) == OW,
              "bn_relu_pool_bwd: dp must be the bf16 (", N, ", ", C, ", ", OH,
              ", ", OW, ") gradient on the input's device");
  TORCH_CHECK(idx.scalar_type() == at::kByte && idx.is_contiguous() &&
                  idx.device() == x.device() && idx.dim() == 4 &&
                  idx.size(0) == N && idx.size(1) == OH && idx.size(2) == OW &&
                  idx.size(3) == C,
              "bn_relu_pool_bwd: idx must be the contiguous uint8 (N, OH, OW, "
              "C) tensor bn_relu_pool_fwd returned, on the input's device");
  bn_check_channel_vec(w, x, C, "weight");
  bn_check_channel_vec(save_mean, x, C, "save_mean");
  bn_check_channel_vec(save_rstd, x, C, "save_rstd");
  dp = dp.contiguous(at::MemoryFormat::ChannelsLast);
  auto opts = x.options().dtype(at::kFloat);
  const int nb = tfosr_bn_pool_blocks((long)N * OH * OW * C);
  auto ws = at::empty({(long)nb * 2 * C}, opts);
  auto dg = at::empty({C}, opts);
  auto db = at::empty({C}, opts);
  auto dx = at::empty_like(x);
  auto s = cur_stream();
  tfosr_bn_relu_pool_bwd_stats(x.data_ptr(), dp.data_ptr(),
                               idx.data_ptr<unsigned char>(),
                               save_mean.data_ptr<float>(),
                               save_rstd.data_ptr<float>(),
                               ws.data_ptr<float>(), nb, N, C, H, W, OH, OW,
                               (int)K, (int)S, (int)P, s);
  tfosr_bn_bwd_merge(ws.data_ptr<float>(), nb, dg.data_ptr<float>(),
                     db.data_ptr<float>(), C, s);
  tfosr_bn_relu_pool_bwd_dx(x.data_ptr(), dp.data_ptr(),
                            idx.data_ptr<unsigned char>(), dx.data_ptr(),
                            save_mean.data_ptr<float>(),
                            save_rstd.data_ptr<float>(), w.data_ptr<float>(),
                            dg.data_ptr<float>(), db.data_ptr<float>(), N, C,
                            H, W, OH, OW, (int)K, (int)S, (int)P, s);
  return {dx, dg, db};
}

// One launch of one kernel of csrc/bn_pool.hip on caller-owned tensors, for
// tools/bn_bench.py --stempool (the two entries above run three launches
// each). family: 0 forward (x -> pooled, idx; mean, rstd, weight, bias),
// 1 bwd stats (x, pooled = dp, idx -> ws of bn_relu_pool_blocks * 2C floats;
// mean, rstd), 2 bwd dx (x, pooled = dp, idx -> out; mean, rstd, weight,
// dgamma, dbeta).
void bn_relu_pool_stage(int family, at::Tensor x, at::Tensor pooled,
                        at::Tensor idx, c10::optional<at::Tensor> out,
                        c10::optional<at::Tensor> ws, std::vector<at::Tensor> p,
                        long K, long S, long P) {
  auto ohw = bn_relu_pool_check("bn_relu_pool_stage", x, K, S, P);
  const int N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int OH = (int)ohw.first, OW = (int)ohw.second;
  const size_t need[3] = {4, 2, 5};
  TORCH_CHECK(family >= 0 && family < 3, "bn_relu_pool_stage: family 0..2");
  TORCH_CHECK(p.size() == need[family], "bn_relu_pool_stage: family ", family,
              " takes ", need[family], " per-channel vectors");
  for (auto& t : p) bn_check_channel_vec(t, x, C, "per-channel vector");
  TORCH_CHECK(pooled.device() == x.device() &&
                  pooled.scalar_type() == at::kBFloat16 && pooled.dim() == 4 &&
                  pooled.size(0) == N && pooled.size(1) == C &&
                  pooled.size(2) == OH && pooled.size(3) == OW &&
                  pooled.is_contiguous(at::MemoryFormat::ChannelsLast),
              "bn_relu_pool_stage: pooled must be bf16 channels_last (N, C, "
              "OH, OW) on the input's device");
  TORCH_CHECK(idx.scalar_type() == at::kByte && idx.is_contiguous() &&
                  idx.device() == x.device() &&
                  idx.numel() == pooled.numel(),
              "bn_relu_pool_stage: idx must hold N*OH*OW*C contiguous bytes");
  const int nb = tfosr_bn_pool_blocks(pooled.numel());
  if (family == 1)
    TORCH_CHECK(ws.has_value() && ws->device() == x.device() &&
                    ws->scalar_type() == at::kFloat && ws->is_contiguous() &&
                    ws->numel() >= (long)nb * 2 * C,
                "bn_relu_pool_stage: ws must hold nb * 2C floats");
  if (family == 2) {
    TORCH_CHECK(out.has_value(), "bn_relu_pool_stage: out is required");
    bn_check_like(*out, x, true, true, "out");
  }
  auto f = [&](size_t i) { return p[i].data_ptr<float>(); };
  auto s = cur_stream();
  unsigned char* ip = idx.data_ptr<unsigned char>();
  switch (family) {
    case 0:
      tfosr_bn_relu_pool_fwd(x.data_ptr(), pooled.data_ptr(), ip, f(0), f(1),
                             f(2), f(3), N, C, H, W, OH, OW, (int)K, (int)S,
                             (int)P, s);
      break;
    case 1:
      tfosr_bn_relu_pool_bwd_stats(x.data_ptr(), pooled.data_ptr(), ip, f(0),
                                   f(1), ws->data_ptr<float>(), nb, N, C, H, W,
                                   OH, OW, (int)K, (int)S, (int)P, s);
      break;
    default:
      tfosr_bn_relu_pool_bwd_dx(x.data_ptr(), pooled.data_ptr(), ip,
                                out->data_ptr(), f(0), f(1), f(2), f(3), f(4),
                                N, C, H, W, OH, OW, (int)K, (int)S, (int)P, s);
  }
}

void sgd_step(at::Tensor p, at::Tensor g, at::Tensor m, double lr, double mu,
              double wd, bool nesterov) {
  check_flat_state("sgd_step", p, {&g, &m});
  tfosr_sgd_step(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(),
                 (float)lr, (float)mu, (float)wd, nesterov, p.numel(),
                 cur_stream());
}

// ---------------------------------------------------------------------------
// Argument checks of the implicit-GEMM conv family and gemm_bt: the kernels
// index raw pointers with sizes narrowed to int, so everything they reach is
// checked here, before any allocation or launch.
// ---------------------------------------------------------------------------

// An activation, gradient or output: 4-D bf16 channels_last on a GPU, every
// size in [1, INT_MAX], C a multiple of cmul (exactly cmul where exact).
void cv_check_act(const char* op, const char* name, const at::Tensor& t,
                  long cmul, bool exact = false) {
  TORCH_CHECK(t.is_cuda(), op, ": ", name, " must be a GPU tensor");
  TORCH_CHECK(t.dim() == 4, op, ": ", name, " must be 4-D (N, C, H, W), got ",
              t.dim(), "-D");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, op, ": ", name,
              " must be bf16, got ", t.scalar_type());
  for (int d = 0; d < 4; ++d)
    TORCH_CHECK(t.size(d) >= 1 && t.size(d) <= INT_MAX, op, ": ", name,
                " has size ", t.size(d), " in dimension ", d,
                ", expected 1 to ", INT_MAX);
  TORCH_CHECK(t.is_contiguous(at::MemoryFormat::ChannelsLast), op, ": ", name,
              " must be channels_last-contiguous");
  TORCH_CHECK(exact ? t.size(1) == cmul : t.size(1) % cmul == 0, op, ": ",
              name, " must have ", exact ? "exactly " : "a multiple of ", cmul,
              " channels, got ", t.size(1));
}

// A second tensor of the call lives on the first one's GPU.
void cv_check_device(const char* op, const char* name, const at::Tensor& t,
                     const at::Tensor& ref) {
  TORCH_CHECK(t.device() == ref.device(), op, ": ", name, " must be on ",
              ref.device(), ", got ", t.device());
}

// The streaming ops (depthwise, transposed-conv head and weight gradient,
// pointwise, bilinear upsampling) take empty tensors and vector-load 16 B.
// What kind of tensor an activation or gradient of theirs is: 4-D on a GPU,
// bf16 (or fp32 where fp32_ok). Returns true when it is empty: nothing to
// launch, and its layout is not looked at.
bool st_check_kind(const char* op, const char* name, const at::Tensor& t,
                   bool fp32_ok) {
  TORCH_CHECK(t.is_cuda(), op, ": ", name, " must be a GPU tensor");
  TORCH_CHECK(t.dim() == 4, op, ": ", name, " must be 4-D (N, C, H, W), got ",
              t.dim(), "-D");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16 ||
                  (fp32_ok && t.scalar_type() == at::kFloat),
              op, ": ", name, fp32_ok ? " must be bf16 or fp32, got "
                                      : " must be bf16, got ",
              t.scalar_type());
  return t.numel() == 0;
}

// st_check_kind, and a tensor that is not empty is channels_last-contiguous
// with its base on the 16 B grid. Each op's own limits follow at the caller.
bool st_check_act(const char* op, const char* name, const at::Tensor& t,
                  bool fp32_ok) {
  if (st_check_kind(op, name, t, fp32_ok)) return true;
  TORCH_CHECK(t.is_contiguous(at::MemoryFormat::ChannelsLast), op, ": ", name,
              " must be channels_last-contiguous");
  TORCH_CHECK((uintptr_t)t.data_ptr() % 16 == 0, op, ": ", name,
              " must be 16-byte aligned");
  return false;
}

// The module's own parameter of a streaming op: on the activation's device,
// contiguous 4-D fp32 (or bf16 where bf16_ok) with a k x k filter. ``what``
// names the shape in the message; the channel relations are the caller's.
void st_check_weight(const char* op, const at::Tensor& w,
                     const at::Tensor& act, bool bf16_ok, long k,
                     const std::string& what) {
  cv_check_device(op, "weight", w, act);
  TORCH_CHECK((w.scalar_type() == at::kFloat ||
               (bf16_ok && w.scalar_type() == at::kBFloat16)) &&
                  w.dim() == 4 && w.size(2) == k && w.size(3) == k &&
                  w.is_contiguous(),
              op, ": weight must be the contiguous ",
              bf16_ok ? "fp32 or bf16 " : "fp32 ", what, ", got ",
              w.scalar_type(), " ", w.sizes());
}

// A weight matrix: 2-D bf16 [rows, cols] on the activation's device (every
// caller passes it 2-D). It need not be contiguous: the entries launch on
// w.contiguous().
void cv_check_weight(const char* op, const char* name, const at::Tensor& w,
                     const at::Tensor& act, long rows, long cols) {
  cv_check_device(op, name, w, act);
  TORCH_CHECK(w.scalar_type() == at::kBFloat16, op, ": ", name,
              " must be bf16, got ", w.scalar_type());
  TORCH_CHECK(w.dim() == 2 && w.size(0) == rows && w.size(1) == cols, op,
              ": ", name, " must be [", rows, ", ", cols,
              "] (output channels x taps * input channels), got ", w.sizes());
}

// gemm_bt and gemm_bf16: c[M, N] = a[M, K] @ b[N, K]^T, a ragged K padded to
// a multiple of 32
at::Tensor gemm_bt_impl(const char* op, at::Tensor a, at::Tensor b,
                        bool out_bf16) {
  TORCH_CHECK(a.is_cuda(), op, ": a must be a GPU tensor");
  cv_check_device(op, "b", b, a);
  TORCH_CHECK(a.scalar_type() == at::kBFloat16 &&
                  b.scalar_type() == at::kBFloat16,
              op, ": a and b must be bf16, got ", a.scalar_type(), " and ",
              b.scalar_type());
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && a.size(1) == b.size(1), op,
              ": expected A[M,K] and B[N,K], got ", a.sizes(), " and ",
              b.sizes());
  TORCH_CHECK(a.size(0) >= 1 && b.size(0) >= 1 && a.size(1) >= 1 &&
                  a.size(0) <= INT_MAX && b.size(0) <= INT_MAX &&
                  a.size(1) <= INT_MAX - 31,
              op, ": M, N and K must be in [1, INT_MAX], got A ", a.sizes(),
              " and B ", b.sizes());
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

at::Tensor gemm_bt(at::Tensor a, at::Tensor b, bool out_bf16) {
  return gemm_bt_impl("gemm_bt", a, b, out_bf16);
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
  TORCH_CHECK(b.dim() == 2, "gemm_bf16: expected A[M,K] and B[K,N], got ",
              a.sizes(), " and ", b.sizes());
  return gemm_bt_impl("gemm_bf16", a, b.t().contiguous(), /*out_bf16=*/false);
}

at::Tensor mfma_probe(at::Tensor a, at::Tensor b) {
  TORCH_CHECK(a.is_cuda(), "mfma_probe: a must be a GPU tensor");
  cv_check_device("mfma_probe", "b", b, a);
  TORCH_CHECK(a.scalar_type() == at::kShort && b.scalar_type() == at::kShort &&
                  a.sizes() == at::IntArrayRef({64, 8}) &&
                  b.sizes() == at::IntArrayRef({64, 8}),
              "mfma_probe: a and b must be [64, 8] int16 lane fragments, got ",
              a.scalar_type(), " ", a.sizes(), " and ", b.scalar_type(), " ",
              b.sizes());
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
#define TFOSR_API_VERSION 15

// Largest filter reach fd*(k-1) the conv entries accept. The kernels form
// ih = oh*S - P + r*fd in int; image coordinates stay below 2^24 in any
// tensor that fits the device, so a reach capped at 2^20 keeps every such
// sum far inside the int range.
static constexpr long kMaxTapReach = 1L << 20;

// Filter geometry of a conv entry: fh x fw taps (at most 49), stride S,
// padding P, input dilation D in {1, 2}, filter dilation fd (> 1 only with
// D == 1). S, P and the tap reach are capped at kMaxTapReach for the reason
// given there.
static void cv_check_filter(const char* op, long fh, long fw, long S, long P,
                            long D, long fd) {
  TORCH_CHECK(fh >= 1 && fw >= 1 && fh * fw <= 49, op,
              ": the filter must be at least 1x1 with at most 49 taps, got ",
              fh, "x", fw);
  TORCH_CHECK(S >= 1 && S <= kMaxTapReach, op, ": stride must be in [1, ",
              kMaxTapReach, "], got ", S);
  TORCH_CHECK(P >= 0 && P <= kMaxTapReach, op, ": padding must be in [0, ",
              kMaxTapReach, "], got ", P);
  TORCH_CHECK(D == 1 || D == 2, op, ": input dilation D must be 1 or 2, got ",
              D);
  TORCH_CHECK(fd >= 1, op, ": filter dilation fd must be >= 1, got ", fd);
  TORCH_CHECK(fd == 1 || D == 1, op,
              ": filter dilation fd > 1 requires input dilation D == 1");
  TORCH_CHECK(fd <= kMaxTapReach && fd * (fh - 1) <= kMaxTapReach &&
                  fd * (fw - 1) <= kMaxTapReach,
              op, ": fd, fd*(fh-1) and fd*(fw-1) must be <= ", kMaxTapReach);
}

// Natural output length of one axis: floor((in_dilated + 2P - reach - 1) / S)
// + 1, or 0 where the dilated filter does not fit the padded input.
static long cv_natural_out(long in, long k, long S, long P, long D, long fd) {
  const long n = (in - 1) * D + 1 + 2 * P - fd * (k - 1) - 1;
  return n < 0 ? 0 : n / S + 1;
}

// The output of an implicit-GEMM launch: OH, OW >= 1, oh * S inside int with
// room for the tap offsets, and the tile count (256-row tiles x the column
// tiles picked from Cout) inside the int the launcher makes the grid from.
static void cv_check_out(const char* op, long N, long Cout, long OH, long OW,
                         long S) {
  TORCH_CHECK(Cout >= 1 && Cout <= INT_MAX, op,
              ": the output needs 1 to ", INT_MAX, " channels, got ", Cout);
  TORCH_CHECK(OH >= 1 && OW >= 1 && OH <= INT_MAX && OW <= INT_MAX, op,
              ": the output size must be at least 1x1, got ", OH, "x", OW);
  TORCH_CHECK((OH - 1) * S <= INT_MAX - 4 * kMaxTapReach &&
                  (OW - 1) * S <= INT_MAX - 4 * kMaxTapReach,
              op, ": output size ", OH, "x", OW, " times stride ", S,
              " exceeds the kernels' 32-bit image coordinates");
  const long bn = Cout >= 192 ? 256 : 128;
  const long ntn = (Cout + bn - 1) / bn;
  TORCH_CHECK(OH <= INT_MAX / OW && N <= INT_MAX / (OH * OW) &&
                  ((N * OH * OW + 255) / 256) <= INT_MAX / ntn,
              op, ": ", N, "x", OH, "x", OW, " output pixels of ", Cout,
              " channels exceed the 32-bit pixel and tile counts");
}

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
  const char* op = stats ? "conv_mfma_stats" : "conv_mfma";
  cv_check_act(op, "x", x, 32);
  cv_check_filter(op, fh, fw, S, P, D, fd);
  long taps = fh * fw;
  int N = x.size(0), Cin = x.size(1), H = x.size(2), W = x.size(3);
  if (OH < 0) {  // the natural size; an explicit one is the dgrad's input size
    OH = cv_natural_out(H, fh, S, P, D, fd);
    OW = cv_natural_out(W, fw, S, P, D, fd);
    TORCH_CHECK(OH >= 1 && OW >= 1, op,
                ": the dilated filter does not fit the padded input");
  }
  cv_check_out(op, N, Cout, OH, OW, S);
  cv_check_weight(op, "wk", wk, x, Cout, taps * Cin);
  auto y = at::empty({N, Cout, OH, OW},
                     x.options().dtype(out_f32 ? at::kFloat : at::kBFloat16),
                     at::MemoryFormat::ChannelsLast);
  const void* guard = zero_guard(x);
  // before either launch, so that a bad TFOS_CONV3X3_TILE is an error on
  // every path; a launch with the statistics epilogue is never eligible
  const ConvTilePlan plan = conv3x3_tile_plan(N, H, W, Cin, Cout, fh, fw, S, P,
                                              D, OH, OW, fd, out_f32, !stats);
  if (stats && D == 1 && !out_f32) {
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
    tfosr_conv3x3_halo(x.data_ptr(), wk.contiguous().data_ptr(), y.data_ptr(),
                       plan.bm, N, H, W, Cin, (int)Cout, cur_stream());
    return {y, c10::nullopt};
  }
  tfosr_conv_mfma(x.data_ptr(), wk.contiguous().data_ptr(), guard,
                  y.data_ptr(), /*out_bf16=*/out_f32 ? 0 : 1, N, H, W, Cin,
                  Cout, OH, OW, S, P, taps, fw, D, 0, (int)fd, cur_stream());
  return {y, c10::nullopt};
}

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
static at::Tensor conv_mfma(at::Tensor x, at::Tensor wk, long Cout, long fh,
                            long fw, long S, long P, long D, long OH, long OW,
                            long fd, bool out_f32) {
  return conv_mfma_impl(x, wk, Cout, fh, fw, S, P, D, OH, OW, fd, out_f32,
                        /*stats=*/false).first;
}

// -> (y, part, rows_per_tile): y is conv_mfma(...) bit for bit; part holds
// y's per-tile BatchNorm partials for bn_fwd_train_pre, or None
// (rows_per_tile 0) where the launch has no statistics epilogue (input
// dilation 2 or fp32 output) and the caller keeps the separate pass.
static py::tuple conv_mfma_stats(at::Tensor x, at::Tensor wk, long Cout,
                                 long fh, long fw, long S, long P, long D,
                                 long OH, long OW, long fd, bool out_f32) {
  auto r = conv_mfma_impl(x, wk, Cout, fh, fw, S, P, D, OH, OW, fd, out_f32,
                          /*stats=*/true);
  if (!r.second.has_value()) return py::make_tuple(r.first, py::none(), 0);
  return py::make_tuple(r.first, *r.second, 256);
}

// Host only: the kernel conv_mfma would launch for this call under the
// current TFOS_CONV3X3_TILE, with its tile, tile count and grid, and the
// largest W the halo kernel can stage (OH/OW < 0: the natural size).
static py::dict conv3x3_halo_plan(long N, long H, long W, long Cin, long Cout,
                                  long fh, long fw, long S, long P, long D,
                                  long OH, long OW, long fd, bool out_f32) {
  TORCH_CHECK(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && S > 0 &&
              fd > 0 && D > 0, "conv3x3_halo_plan: bad dims");
  if (OH < 0) {
    OH = cv_natural_out(H, fh, S, P, D, fd);
    OW = cv_natural_out(W, fw, S, P, D, fd);
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
}

// conv_mfma accumulating INTO an existing channels_last tensor:
// out += conv(x, wk) — fuses the residual-join gradient accumulation the
// eager autograd would do as a separate whole-tensor add (8.4 ms/step of
// CUDAFunctor_add at ResNet-50 b1024, profiles/README r01).
static at::Tensor conv_mfma_acc(at::Tensor x, at::Tensor wk, at::Tensor out,
                                long fh, long fw, long S, long P, long D) {
  const char* op = "conv_mfma_acc";
  cv_check_act(op, "x", x, 32);
  cv_check_act(op, "out", out, 1);
  cv_check_device(op, "out", out, x);
  cv_check_filter(op, fh, fw, S, P, D, /*fd=*/1);
  int N = x.size(0), Cin = x.size(1), H = x.size(2), W = x.size(3);
  long taps = fh * fw;
  long Cout = out.size(1), OH = out.size(2), OW = out.size(3);
  TORCH_CHECK(out.size(0) == N, op, ": out must have x's batch ", N, ", got ",
              out.size(0));
  cv_check_out(op, N, Cout, OH, OW, S);
  cv_check_weight(op, "wk", wk, x, Cout, taps * Cin);
  const void* guard = zero_guard(x);
  tfosr_conv_mfma(x.data_ptr(), wk.contiguous().data_ptr(), guard,
                  out.data_ptr(), /*out_bf16=*/1, N, H, W, Cin, Cout, OH, OW,
                  S, P, taps, fw, D, 1, /*fd=*/1, cur_stream());
  return out;
}

// One parity class of a stride-2 backward-data / transposed conv:
// out[oh*2+oh0, ow*2+ow0] = conv(x, wk_class) with the class's taps
// (list of (r,s) pairs). wk_class: [Cout, ntaps*Cin]. Writes into `out`
// (pre-allocated [N, Cout, OHr, OWr] channels_last; classes disjoint).
static at::Tensor conv_par(at::Tensor x, at::Tensor wk, at::Tensor out,
                           std::vector<long> taps_r, std::vector<long> taps_s,
                           long P, bool accum) {
  const char* op = "conv_par";
  cv_check_act(op, "x", x, 32);
  cv_check_act(op, "out", out, 1);
  cv_check_device(op, "out", out, x);
  int N = x.size(0), Cin = x.size(1), H = x.size(2), W = x.size(3);
  TORCH_CHECK(out.size(0) == N, op, ": out must have x's batch ", N, ", got ",
              out.size(0));
  long ntaps = (long)taps_r.size();
  TORCH_CHECK(ntaps >= 1 && ntaps <= 8 && taps_s.size() == (size_t)ntaps, op,
              ": taps_r and taps_s must be equally long lists of 1 to 8 "
              "taps, got ", taps_r.size(), " and ", taps_s.size());
  TORCH_CHECK(P >= 0 && P <= kMaxTapReach, op, ": padding must be in [0, ",
              kMaxTapReach, "], got ", P);
  // the output parity (oh0, ow0) of the class follows from any of its taps:
  // ihv = (oh*2+oh0) - P + r must be even, so every tap has one parity; a
  // tap is packed into four bits each of r and s
  for (long i = 0; i < ntaps; ++i) {
    TORCH_CHECK(taps_r[i] >= 0 && taps_r[i] <= 15 && taps_s[i] >= 0 &&
                    taps_s[i] <= 15,
                op, ": tap (", taps_r[i], ", ", taps_s[i],
                ") is outside [0, 15]");
    TORCH_CHECK(taps_r[i] % 2 == taps_r[0] % 2 &&
                    taps_s[i] % 2 == taps_s[0] % 2,
                op, ": tap (", taps_r[i], ", ", taps_s[i],
                ") is not in the parity class of tap (", taps_r[0], ", ",
                taps_s[0], ")");
  }
  long Cout = out.size(1), OHr = out.size(2), OWr = out.size(3);
  cv_check_weight(op, "wk", wk, x, Cout, ntaps * Cin);
  long oh0 = ((P - taps_r[0]) % 2 + 2) % 2;
  long ow0 = ((P - taps_s[0]) % 2 + 2) % 2;
  long OHs = (OHr - oh0 + 1) / 2, OWs = (OWr - ow0 + 1) / 2;
  if (OHs <= 0 || OWs <= 0) return out;
  cv_check_out(op, N, Cout, OHs, OWs, /*S=*/2);
  unsigned long pack = 0;
  for (long i = 0; i < ntaps; ++i)
    pack |= ((unsigned long)((taps_r[i] << 4) | taps_s[i])) << (i * 8);
  const void* guard = zero_guard(x);
  tfosr_conv_par(x.data_ptr(), wk.contiguous().data_ptr(), guard,
                 out.data_ptr(), N, H, W, Cin, (int)Cout, (int)OHs,
                 (int)OWs, (int)P, (int)ntaps, pack, (int)oh0, (int)ow0,
                 (int)OWr, OHr * OWr, accum ? 1 : 0, cur_stream());
  return out;
}

// ResNet stem: 7x7/s2/p3 conv over a pre-padded NHWC4 image
// ([N,4,230,230] channels_last bf16, Cin 3->4 zero-padded, spatial pad 3
// baked in); weight pre-packed to [Cout, 7*32] with zero columns for the
// pads. Output [N, Cout, 112, 112].
static at::Tensor conv_stem(at::Tensor x4, at::Tensor w224, long Cout) {
  const char* op = "conv_stem";
  cv_check_act(op, "x4", x4, 4, /*exact=*/true);
  int N = x4.size(0), Hp = x4.size(2), Wp = x4.size(3);
  TORCH_CHECK(Hp >= 7 && Wp >= 7, op, ": the padded image must be at least "
              "7x7, got ", Hp, "x", Wp);
  int OH = cv_natural_out(Hp, 7, 2, 0, 1, 1);
  int OW = cv_natural_out(Wp, 7, 2, 0, 1, 1);
  cv_check_out(op, N, Cout, OH, OW, /*S=*/2);
  cv_check_weight(op, "w224", w224, x4, Cout, 224);
  auto y = at::empty({N, Cout, OH, OW}, x4.options(),
                     at::MemoryFormat::ChannelsLast);
  const void* guard = zero_guard(x4);
  tfosr_conv_stem(x4.data_ptr(), w224.contiguous().data_ptr(),
                  guard, y.data_ptr(), N, Hp, Wp, Cout, OH, OW,
                  cur_stream());
  return y;
}

// The weight-gradient entries take dy of the forward's natural output size
// for x and the given filter, with x's batch; M = N*OH*OW <= INT_MAX.
static void cv_check_wrw_pair(const char* op, const at::Tensor& dy,
                              const at::Tensor& x, long xc, bool x_exact,
                              long R, long S_f, long stride, long P,
                              long fd) {
  cv_check_act(op, "dy", dy, 8);
  cv_check_act(op, "x", x, xc, x_exact);
  cv_check_device(op, "x", x, dy);
  cv_check_filter(op, R, S_f, stride, P, /*D=*/1, fd);
  const long N = x.size(0);
  const long OH = cv_natural_out(x.size(2), R, stride, P, 1, fd);
  const long OW = cv_natural_out(x.size(3), S_f, stride, P, 1, fd);
  TORCH_CHECK(dy.size(0) == N && dy.size(2) == OH && dy.size(3) == OW, op,
              ": x ", x.sizes(), " with a ", R, "x", S_f, " filter, stride ",
              stride, ", padding ", P, ", dilation ", fd,
              " gives a gradient of [", N, ", Cout, ", OH, ", ", OW,
              "], got ", dy.sizes());
  TORCH_CHECK(OH <= INT_MAX / OW && N <= INT_MAX / (OH * OW), op, ": ", N,
              "x", OH, "x", OW, " gradient pixels exceed the kernels' 32-bit "
              "pixel index");
}

// wrw v2: MFMA + hardware transpose-reads + split-M workspace.
// dy [N,Cout,OH,OW] cl, x [N,Cin,H,W] cl; filter R x S_f, conv stride,
// pad P. Returns fp32 dW [Cout, R*S_f*Cin].
// fd: filter dilation of the 3x3 case (dW tap (r, s) pairs dy[oh, ow]
// with x[oh*stride - P + r*fd, ow*stride - P + s*fd]).
static at::Tensor conv_wrw2(at::Tensor dy, at::Tensor x, long R, long S_f,
                            long stride, long P, long fd) {
  const char* op = "conv_wrw2";
  long taps = R * S_f;
  TORCH_CHECK(taps == 1 || taps == 9, op, " supports 1x1 and 3x3, got ", R,
              "x", S_f);
  TORCH_CHECK(fd >= 1, op, ": filter dilation fd must be >= 1, got ", fd);
  TORCH_CHECK(taps != 1 || fd == 1, op,
              ": a 1x1 filter has no dilation, fd must be 1");
  // the 1x1 kernel reads x at (oh*stride, ow*stride) with no padding test
  TORCH_CHECK(taps != 1 || P == 0, op,
              ": a 1x1 filter takes no padding, P must be 0, got ", P);
  cv_check_wrw_pair(op, dy, x, 8, false, R, S_f, stride, P, fd);
  int N = x.size(0), Cin = x.size(1), H = x.size(2), W = x.size(3);
  int Cout = dy.size(1), OH = dy.size(2), OW = dy.size(3);
  long M = (long)N * OH * OW;
  int split = tfosr_wrw2_split(Cout, Cin, M);
  long K = taps * (long)Cin;
  // the split reduce indexes the workspace with 32-bit offsets
  TORCH_CHECK((long)split * Cout * K < (1L << 32), op,
              ": the split workspace exceeds 2^32 elements");
  auto ws = at::empty({(long)split, (long)Cout * K},
                      x.options().dtype(at::kFloat));
  auto dW = at::empty({(long)Cout, K}, x.options().dtype(at::kFloat));
  const void* guard = zero_guard(x);
  tfosr_conv_wrw2(dy.data_ptr(), x.data_ptr(), guard,
                  ws.data_ptr<float>(), dW.data_ptr<float>(), N, H, W, Cin,
                  Cout, OH, OW, R, S_f, stride, P, split, (int)fd,
                  cur_stream());
  return dW;
}

// stem weight gradient over the same NHWC4 padded view: returns fp32
// [Cout, 7*32] (rows x (8 px x 4 ch), pads included — caller unpacks)
static at::Tensor conv_stem_wrw(at::Tensor dy, at::Tensor x4) {
  const char* op = "conv_stem_wrw";
  // the geometry is the 7x7 filter's; the kernel sees its rows as 7 taps
  cv_check_wrw_pair(op, dy, x4, 4, true, /*R=*/7, /*S_f=*/7, /*stride=*/2,
                    /*P=*/0, /*fd=*/1);
  int N = x4.size(0), Hp = x4.size(2), Wp = x4.size(3);
  int Cout = dy.size(1), OH = dy.size(2), OW = dy.size(3);
  long M = (long)N * OH * OW;
  int split = tfosr_wrw2_split(Cout, 32, M);
  long K = 7L * 32;
  TORCH_CHECK((long)split * Cout * K < (1L << 32), op,
              ": the split workspace exceeds 2^32 elements");
  auto ws = at::empty({(long)split, (long)Cout * K},
                      x4.options().dtype(at::kFloat));
  auto dW = at::empty({(long)Cout, K}, x4.options().dtype(at::kFloat));
  const void* guard = zero_guard(x4);
  tfosr_conv_wrw2(dy.data_ptr(), x4.data_ptr(), guard,
                  ws.data_ptr<float>(), dW.data_ptr<float>(), N, Hp, Wp,
                  /*Cin=*/32, Cout, OH, OW, /*R=*/7, /*S_f=*/1,
                  /*stride=*/2, /*P=*/0, split, /*fd=*/1, cur_stream());
  return dW;
}

// The round-1 TN weight-gradient kernel (stride 1, undilated), kept as the
// TFOS_WRW=mfma backend. Returns fp32 dW [Cout, R*S*Cin].
static at::Tensor conv_wrw(at::Tensor dy, at::Tensor x, long R, long S,
                           long P) {
  cv_check_wrw_pair("conv_wrw", dy, x, 8, false, R, S, /*stride=*/1, P,
                    /*fd=*/1);
  int N = x.size(0), Cin = x.size(1), H = x.size(2), W = x.size(3);
  int Cout = dy.size(1), OH = dy.size(2), OW = dy.size(3);
  auto dW = at::zeros({Cout, R * S * (long)Cin},
                      x.options().dtype(at::kFloat));
  tfosr_conv_wrw(dy.data_ptr(), x.data_ptr(), dW.data_ptr<float>(), N, H, W,
                 Cin, Cout, OH, OW, R, S, P, cur_stream());
  return dW;
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
  if (st_check_act(op, name, t, true)) return true;
  const int V = dw_vec(t);
  TORCH_CHECK(t.size(1) % V == 0, op, ": C=", t.size(1),
              " must be a multiple of ", V, " for ", t.scalar_type());
  TORCH_CHECK(t.numel() / V < (1L << 31), op, ": ", name, " has ", t.numel(),
              " elements, more than the kernels index");
  return false;
}

static void dw_check_weight(const char* op, const at::Tensor& w,
                            const at::Tensor& act) {
  const std::string what =
      "[C,1,3,3] parameter with C=" + std::to_string(act.size(1));
  st_check_weight(op, w, act, false, 3, what);
  TORCH_CHECK(w.size(0) == act.size(1) && w.size(1) == 1, op,
              ": weight must be the contiguous fp32 ", what, ", got ",
              w.scalar_type(), " ", w.sizes());
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

// ---------------------------------------------------------------------------
// Transposed-conv head (csrc/convt_head.hip): k4 s2 p1, Cin % 8 == 0 in
// [8, 256], Cout in [1, 8], bf16 channels_last
// ---------------------------------------------------------------------------

// An activation or gradient as the kernels take it. Returns true when the
// tensor is empty (nothing to launch).
static bool cth_check_act(const char* op, const char* name,
                          const at::Tensor& t) {
  if (st_check_act(op, name, t, false)) return true;
  TORCH_CHECK(t.numel() < (1L << 31), op, ": ", name, " has ", t.numel(),
              " elements, more than the kernels index");
  return false;
}

static void cth_check_channels(const char* op, long Cin, long Cout) {
  TORCH_CHECK(Cin % 8 == 0 && Cin >= 8 && Cin <= 256, op, ": Cin=", Cin,
              " must be a multiple of 8 in [8, 256]");
  TORCH_CHECK(Cout >= 1 && Cout <= 8, op, ": Cout=", Cout,
              " must be in [1, 8]");
}

static void cth_check_weight(const char* op, const at::Tensor& w,
                             const at::Tensor& act) {
  st_check_weight(op, w, act, false, 4, "[Cin,Cout,4,4] parameter");
}

static at::Tensor convt_head_fwd(at::Tensor x, at::Tensor w,
                                 c10::optional<at::Tensor> bias) {
  const char* op = "convt_head_fwd";
  const bool empty = cth_check_act(op, "x", x);
  cth_check_weight(op, w, x);
  const long N = x.size(0), Cin = x.size(1), H = x.size(2), W = x.size(3);
  const long Cout = w.size(1);
  TORCH_CHECK(w.size(0) == Cin, op, ": weight must be [Cin,Cout,4,4] with "
              "Cin=", Cin, ", got ", w.sizes());
  cth_check_channels(op, Cin, Cout);
  const float* bp = nullptr;
  if (bias.has_value() && bias->defined()) {
    TORCH_CHECK(bias->device() == x.device() &&
                    bias->scalar_type() == at::kFloat && bias->dim() == 1 &&
                    bias->size(0) == Cout && bias->is_contiguous(),
                op, ": bias must be the contiguous fp32 [Cout] parameter on ",
                x.device(), " with Cout=", Cout, ", got ",
                bias->scalar_type(), " ", bias->sizes(), " on ",
                bias->device());
    bp = bias->data_ptr<float>();
  }
  auto y = at::empty({N, Cout, 2 * H, 2 * W}, x.options(),
                     at::MemoryFormat::ChannelsLast);
  if (empty) return y;
  TORCH_CHECK(y.numel() < (1L << 31), op, ": y has ", y.numel(),
              " elements, more than the kernels index");
  tfosr_convt_head_fwd(x.data_ptr(), w.data_ptr<float>(), bp, y.data_ptr(), N,
                       Cin, Cout, H, W, cur_stream());
  return y;
}

static at::Tensor convt_head_dgrad(at::Tensor dy, at::Tensor w, long H,
                                   long W) {
  const char* op = "convt_head_dgrad";
  const bool empty = cth_check_act(op, "dy", dy);
  cth_check_weight(op, w, dy);
  TORCH_CHECK(H >= 0 && W >= 0, op, ": H and W must not be negative");
  const long N = dy.size(0), Cout = dy.size(1), Cin = w.size(0);
  TORCH_CHECK(w.size(1) == Cout, op, ": weight must be [Cin,Cout,4,4] with "
              "Cout=", Cout, ", got ", w.sizes());
  cth_check_channels(op, Cin, Cout);
  TORCH_CHECK(dy.size(2) == 2 * H && dy.size(3) == 2 * W, op, ": a ", H, "x",
              W, " input gives ", 2 * H, "x", 2 * W, ", the gradient is ",
              dy.size(2), "x", dy.size(3));
  auto dx = at::empty({N, Cin, H, W}, dy.options(),
                      at::MemoryFormat::ChannelsLast);
  if (empty || dx.numel() == 0) return dx;
  TORCH_CHECK(dx.numel() < (1L << 31), op, ": dx has ", dx.numel(),
              " elements, more than the kernels index");
  tfosr_convt_head_dgrad(dy.data_ptr(), w.data_ptr<float>(), dx.data_ptr(), N,
                         Cin, Cout, H, W, cur_stream());
  return dx;
}

static std::tuple<at::Tensor, at::Tensor> convt_head_wrw(at::Tensor dy,
                                                         at::Tensor x) {
  const char* op = "convt_head_wrw";
  const bool dy_empty = cth_check_act(op, "dy", dy);
  const bool x_empty = cth_check_act(op, "x", x);
  TORCH_CHECK(x.device() == dy.device(), op, ": x must be on ", dy.device(),
              ", got ", x.device());
  const long N = x.size(0), Cin = x.size(1), H = x.size(2), W = x.size(3);
  const long Cout = dy.size(1);
  cth_check_channels(op, Cin, Cout);
  TORCH_CHECK(dy.size(0) == N && dy.size(2) == 2 * H && dy.size(3) == 2 * W,
              op, ": x ", x.sizes(), " gives a gradient of [", N, ", Cout, ",
              2 * H, ", ", 2 * W, "], got ", dy.sizes());
  auto opts = x.options().dtype(at::kFloat);
  if (dy_empty || x_empty)
    return {at::zeros({Cin, Cout, 4, 4}, opts), at::zeros({Cout}, opts)};
  int nblk;
  long slab;
  tfosr_convt_head_wrw_plan(N * H * W, (int)Cin, (int)Cout, &nblk, &slab);
  auto part = at::empty({(long)nblk, Cin * 16 * Cout + Cout}, opts);
  auto dw = at::empty({Cin, Cout, 4, 4}, opts);
  auto db = at::empty({Cout}, opts);
  tfosr_convt_head_wrw(dy.data_ptr(), x.data_ptr(), part.data_ptr<float>(),
                       dw.data_ptr<float>(), db.data_ptr<float>(), N, Cin,
                       Cout, H, W, cur_stream());
  return {dw, db};
}

// ---------------------------------------------------------------------------
// Transposed-conv weight gradient (csrc/convt_wrw.hip): k4 s2 p1,
// output_padding 0, channel counts that are multiples of 8, bf16 channels_last
// ---------------------------------------------------------------------------

// x or dy as the kernel takes it: the cv_check_act conditions, except that a
// pixel may be wider than C (a channel slice of a channels_last tensor keeps
// its parent's pixel stride). Returns the pixel stride in elements.
static long ctw_check_act(const char* op, const char* name,
                          const at::Tensor& t) {
  const long C = t.size(1), H = t.size(2), W = t.size(3);
  long ps = C;
  if (!t.is_contiguous(at::MemoryFormat::ChannelsLast)) {
    ps = t.stride(3);
    TORCH_CHECK(t.stride(1) == 1 && ps >= C && ps % 8 == 0 &&
                    t.stride(2) == W * ps && t.stride(0) == H * W * ps,
                op, ": ", name, " must be channels_last-contiguous, or a "
                "channel slice of such a tensor with a pixel stride that is a "
                "multiple of 8; got sizes ", t.sizes(), " strides ",
                t.strides());
  }
  for (int d = 0; d < 4; ++d)
    TORCH_CHECK(t.size(d) <= INT_MAX, op, ": ", name, " has size ", t.size(d),
                " in dimension ", d, ", expected at most ", INT_MAX);
  TORCH_CHECK(C % 8 == 0, op, ": ", name, " must have a multiple of 8 "
              "channels, got ", C);
  TORCH_CHECK((uintptr_t)t.data_ptr() % 16 == 0, op, ": ", name,
              " must be 16-byte aligned");
  return ps;
}

static py::dict convt_wrw_plan(long N, long H, long W, long Cin, long Cout) {
  TORCH_CHECK(N > 0 && H > 0 && W > 0 && N * H <= INT_MAX && 2 * H <= INT_MAX &&
                  2 * W <= INT_MAX,
              "convt_wrw_plan: N, H and W must be positive, with N*H, 2H and "
              "2W at most ", INT_MAX);
  TORCH_CHECK(Cin > 0 && Cout > 0 && Cin % 8 == 0 && Cout % 8 == 0 &&
                  Cin <= INT_MAX && Cout <= INT_MAX &&
                  Cin * Cout <= INT_MAX / 16,
              "convt_wrw_plan: Cin and Cout must be positive multiples of 8 "
              "with Cin*Cout*16 at most ", INT_MAX);
  int rb = 0, rows = 0, slabs = 0, tiles = 0, grid = 0, lds = 0;
  long ws = 0;
  const int ok = tfosr_convt_wrw_plan(N, (int)H, (int)W, (int)Cin, (int)Cout,
                                      &rb, &rows, &slabs, &tiles, &grid, &ws,
                                      &lds);
  py::dict d;
  d["eligible"] = (bool)ok;
  d["block_rows"] = rb;
  d["slab_rows"] = rows;
  d["slabs"] = slabs;
  d["tiles"] = tiles;
  d["grid"] = grid;
  d["ws_bytes"] = ws;
  d["lds_bytes"] = lds;
  return d;
}

static at::Tensor convt_wrw(at::Tensor dy, at::Tensor x) {
  const char* op = "convt_wrw";
  // the layout is ctw_check_act's: a channel slice passes here
  const bool dy_empty = st_check_kind(op, "dy", dy, false);
  const bool x_empty = st_check_kind(op, "x", x, false);
  cv_check_device(op, "x", x, dy);
  const long N = x.size(0), Cin = x.size(1), H = x.size(2), W = x.size(3);
  const long Cout = dy.size(1);
  TORCH_CHECK(dy.size(0) == N && dy.size(2) == 2 * H && dy.size(3) == 2 * W,
              op, ": x ", x.sizes(), " gives a gradient of [", N, ", Cout, ",
              2 * H, ", ", 2 * W, "], got ", dy.sizes());
  auto opts = x.options().dtype(at::kFloat);
  if (dy_empty || x_empty) return at::zeros({Cin, Cout, 4, 4}, opts);
  const long dps = ctw_check_act(op, "dy", dy);
  const long xps = ctw_check_act(op, "x", x);
  const py::dict plan = convt_wrw_plan(N, H, W, Cin, Cout);
  TORCH_CHECK(plan["eligible"].cast<bool>(), op, ": W=", W,
              " is wider than one staged row block holds");
  const long wsb = plan["ws_bytes"].cast<long>();
  auto dw = at::empty({Cin, Cout, 4, 4}, opts);
  at::Tensor ws;
  if (wsb > 0) ws = at::empty({wsb / 4}, opts);
  const hipError_t err = tfosr_convt_wrw(
      x.data_ptr(), dy.data_ptr(), wsb > 0 ? ws.data_ptr<float>() : nullptr,
      dw.data_ptr<float>(), N, (int)H, (int)W, (int)Cin, (int)Cout, xps, dps,
      cur_stream());
  TORCH_CHECK(err == hipSuccess, op, ": launch failed: ",
              hipGetErrorString(err));
  return dw;
}

// ---------------------------------------------------------------------------
// Pointwise convs (csrc/pwconv.hip): 1x1, stride 1, no bias, channel counts
// that are multiples of 8 in [8, 960], bf16 channels_last; the weight is the
// module's contiguous [Cout, Cin, 1, 1] parameter, fp32 or bf16
// ---------------------------------------------------------------------------

struct PwPlan {
  int tile_m, panels, ppp, grid, lds_bytes;
  long m_tiles;
};

static PwPlan pw_plan(long M, long K, long Co) {
  PwPlan p;
  tfosr_pwconv_plan(M, (int)K, (int)Co, &p.tile_m, &p.m_tiles, &p.panels,
                    &p.ppp, &p.grid, &p.lds_bytes);
  return p;
}

static void pw_check_channels(const char* op, const char* name, long C) {
  int tile_m, max_grid, max_c;
  tfosr_pwconv_info(&tile_m, &max_grid, &max_c);
  TORCH_CHECK(C % 8 == 0 && C >= 8 && C <= max_c, op, ": ", name, "=", C,
              " must be a multiple of 8 in [8, ", max_c, "]");
}

// An activation or gradient as the kernels take it. Returns true when the
// tensor is empty (nothing to launch); one that is not also meets
// cv_check_act's size limits, and N*H*W fits the kernels' 32-bit pixel index.
static bool pw_check_act(const char* op, const char* name,
                         const at::Tensor& t) {
  if (st_check_act(op, name, t, false)) return true;
  cv_check_act(op, name, t, 8);
  pw_check_channels(op, name, t.size(1));
  TORCH_CHECK(t.numel() / t.size(1) <= INT_MAX, op, ": ", name, " has ",
              t.numel() / t.size(1), " pixels, more than the 32-bit pixel "
              "index holds");
  return false;
}

static void pw_check_weight(const char* op, const at::Tensor& w,
                            const at::Tensor& act) {
  st_check_weight(op, w, act, true, 1, "[Cout,Cin,1,1] parameter");
  pw_check_channels(op, "Cout", w.size(0));
  pw_check_channels(op, "Cin", w.size(1));
}

// fwd (transposed = false): y[N, Cout, H, W] from x[N, Cin, H, W]; dgrad
// (transposed = true): dx[N, Cin, H, W] from dy[N, Cout, H, W]
static at::Tensor pw_gemm(const char* op, const char* name, at::Tensor in,
                          at::Tensor w, bool transposed) {
  const bool empty = pw_check_act(op, name, in);
  pw_check_weight(op, w, in);
  const long K = w.size(transposed ? 0 : 1), Co = w.size(transposed ? 1 : 0);
  TORCH_CHECK(in.size(1) == K, op, ": weight must be [Cout,Cin,1,1] with ",
              transposed ? "Cout=" : "Cin=", in.size(1), ", got ", w.sizes());
  auto out = at::empty({in.size(0), Co, in.size(2), in.size(3)}, in.options(),
                       at::MemoryFormat::ChannelsLast);
  if (empty) return out;
  const long M = in.size(0) * in.size(2) * in.size(3);
  const hipError_t err = tfosr_pwconv_gemm(
      in.data_ptr(), w.data_ptr(), w.scalar_type() == at::kBFloat16,
      out.data_ptr(), M, (int)K, (int)Co, transposed, cur_stream());
  TORCH_CHECK(err == hipSuccess, op, ": launch failed: ",
              hipGetErrorString(err));
  return out;
}

static at::Tensor pwconv_fwd(at::Tensor x, at::Tensor w) {
  return pw_gemm("pwconv_fwd", "x", x, w, false);
}

static at::Tensor pwconv_dgrad(at::Tensor dy, at::Tensor w) {
  return pw_gemm("pwconv_dgrad", "dy", dy, w, true);
}

// ---------------------------------------------------------------------------
// Bilinear upsampling (csrc/upsample_bilinear.hip): channels_last bf16 or
// fp32, C in [1, 2048], upscale or identity on both axes
// ---------------------------------------------------------------------------

struct UbPlan {
  int fwd_cc, fwd_ph, fwd_pw, bwd_cc, bwd_p;
  long fwd_tiles, bwd_tiles;
};

static int ub_max_c() {
  int v[9];
  tfosr_upsample_bilinear_info(v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6,
                               v + 7, v + 8);
  return v[8];
}

// The tensor as the kernels take it. Returns true when it is empty, which an
// image without rows or columns is not allowed to be.
static bool ub_check_act(const char* op, const char* name,
                         const at::Tensor& t) {
  const bool empty = st_check_act(op, name, t, true);
  TORCH_CHECK(t.size(2) >= 1 && t.size(3) >= 1, op, ": ", name,
              " must have at least one row and column, got ", t.sizes());
  if (empty) return true;
  TORCH_CHECK(t.size(1) <= ub_max_c(), op, ": C=", t.size(1),
              " must be at most ", ub_max_c());
  return false;
}

// Sizes of the small (in) and large (out) image of one call; fills the plan.
static UbPlan ub_check_sizes(const char* op, long N, long C, long Hin,
                             long Win, long Hout, long Wout, bool align,
                             int itemsize) {
  TORCH_CHECK(Hout >= 1 && Hout <= INT_MAX && Wout >= 1 && Wout <= INT_MAX &&
                  Hin >= 1 && Hin <= INT_MAX && Win >= 1 && Win <= INT_MAX,
              op, ": sizes must be in [1, ", INT_MAX, "], got ", Hin, "x", Win,
              " and ", Hout, "x", Wout);
  TORCH_CHECK(Hout >= Hin && Wout >= Win, op, ": upscale only, got ", Hin,
              "x", Win, " -> ", Hout, "x", Wout);
  TORCH_CHECK(N * Hout <= INT_MAX / Wout, op, ": ", N, "x", Hout, "x", Wout,
              " pixels, more than the kernels index");
  UbPlan p{};
  if (C == 0) return p;
  tfosr_upsample_bilinear_plan((int)C, (int)Hin, (int)Win, (int)Hout,
                               (int)Wout, align, itemsize, &p.fwd_cc,
                               &p.fwd_ph, &p.fwd_pw, &p.fwd_tiles, &p.bwd_cc,
                               &p.bwd_p, &p.bwd_tiles);
  TORCH_CHECK(N == 0 || (p.fwd_tiles <= INT_MAX / N &&
                         p.bwd_tiles <= INT_MAX / N),
              op, ": ", N, " images of ", p.fwd_tiles, " and ", p.bwd_tiles,
              " tiles, more than the kernels index");
  return p;
}

static at::Tensor upsample_bilinear_fwd(at::Tensor x, long Hout, long Wout,
                                        bool align_corners) {
  const char* op = "upsample_bilinear_fwd";
  const bool empty = ub_check_act(op, "x", x);
  const long N = x.size(0), C = x.size(1), Hin = x.size(2), Win = x.size(3);
  ub_check_sizes(op, N, C, Hin, Win, Hout, Wout, align_corners,
                 (int)x.element_size());
  auto y = at::empty({N, C, Hout, Wout}, x.options(),
                     at::MemoryFormat::ChannelsLast);
  if (empty) return y;
  tfosr_upsample_bilinear_fwd(x.data_ptr(), y.data_ptr(),
                              x.scalar_type() == at::kBFloat16, (int)N, (int)C,
                              (int)Hin, (int)Win, (int)Hout, (int)Wout,
                              align_corners, cur_stream());
  return y;
}

static at::Tensor upsample_bilinear_bwd(at::Tensor dy, long Hin, long Win,
                                        bool align_corners) {
  const char* op = "upsample_bilinear_bwd";
  const bool empty = ub_check_act(op, "dy", dy);
  const long N = dy.size(0), C = dy.size(1), Hout = dy.size(2),
             Wout = dy.size(3);
  ub_check_sizes(op, N, C, Hin, Win, Hout, Wout, align_corners,
                 (int)dy.element_size());
  auto dx = at::empty({N, C, Hin, Win}, dy.options(),
                      at::MemoryFormat::ChannelsLast);
  if (empty) return dx;
  tfosr_upsample_bilinear_bwd(dy.data_ptr(), dx.data_ptr(),
                              dy.scalar_type() == at::kBFloat16, (int)N,
                              (int)C, (int)Hin, (int)Win, (int)Hout, (int)Wout,
                              align_corners, cur_stream());
  return dx;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("api_version", []() { return TFOSR_API_VERSION; });
  m.def("upsample_bilinear_fwd", &upsample_bilinear_fwd, py::arg("x"),
        py::arg("Hout"), py::arg("Wout"), py::arg("align_corners"));
  m.def("upsample_bilinear_bwd", &upsample_bilinear_bwd, py::arg("dy"),
        py::arg("Hin"), py::arg("Win"), py::arg("align_corners"));
  m.def("upsample_bilinear_info", []() {
    int block, max_grid, fh, fw, bh, bw, br, lds, max_c;
    tfosr_upsample_bilinear_info(&block, &max_grid, &fh, &fw, &bh, &bw, &br,
                                 &lds, &max_c);
    py::dict d;
    d["block"] = block;
    d["max_grid"] = max_grid;
    d["fwd_tile_h"] = fh;
    d["fwd_tile_w"] = fw;
    d["bwd_tile_h"] = bh;
    d["bwd_tile_w"] = bw;
    d["bwd_rows"] = br;
    d["lds"] = lds;
    d["max_c"] = max_c;
    return d;
  });
  m.def("upsample_bilinear_plan", [](long C, long Hin, long Win, long Hout,
                                     long Wout, bool align_corners,
                                     long itemsize) {
    TORCH_CHECK(C >= 1 && C <= ub_max_c() && (itemsize == 2 || itemsize == 4),
                "upsample_bilinear_plan: C must be in [1, ", ub_max_c(),
                "] and itemsize 2 or 4");
    const UbPlan p = ub_check_sizes("upsample_bilinear_plan", 1, C, Hin, Win,
                                    Hout, Wout, align_corners, (int)itemsize);
    py::dict d;
    d["fwd_cc"] = p.fwd_cc;
    d["fwd_patch_h"] = p.fwd_ph;
    d["fwd_patch_w"] = p.fwd_pw;
    d["fwd_tiles"] = p.fwd_tiles;
    d["bwd_cc"] = p.bwd_cc;
    d["bwd_cols"] = p.bwd_p;
    d["bwd_tiles"] = p.bwd_tiles;
    return d;
  });
  m.def("bn_fwd_train", &bn_fwd_train);
  m.def("bn_fwd_eval", &bn_fwd_eval);
  m.def("bn_bwd", &bn_bwd);
  m.def("bn_relu_pool_eligible", &bn_relu_pool_eligible, py::arg("x"),
        py::arg("K"), py::arg("S"), py::arg("P"));
  m.def("bn_relu_pool_fwd", &bn_relu_pool_fwd);
  m.def("bn_relu_pool_bwd", &bn_relu_pool_bwd);
  m.def("bn_relu_pool_stage", &bn_relu_pool_stage);
  m.def("bn_relu_pool_blocks", [](long pooled_numel) {
    TORCH_CHECK(pooled_numel >= 0, "bn_relu_pool_blocks: negative size");
    return tfosr_bn_pool_blocks(pooled_numel);
  });
  m.def("bn_dual_eligible", &bn_dual_eligible);
  m.def("bn_dual_fwd_train", &bn_dual_fwd_train);
  m.def("bn_dual_bwd", &bn_dual_bwd);
  // blocks of the fast-path reduction kernels for a shape (0 = generic path):
  // tools/bn_bench.py counts the partials' bytes with it
  m.def("bn_fast_blocks", [](long total, int C, bool bf16, bool nhwc) {
    return tfosr_bn_fast_blocks(total, C, bf16, nhwc);
  });
  // the row tier's launch shape for a tensor of `total` elements: (reduction
  // blocks, pixel lanes, threads per block); blocks == 0: not the row tier
  m.def("bn_rows_plan", [](long total, int C, bool bf16, bool nhwc) {
    const BNTier t = bn_tier(total, C, bf16, nhwc);
    return t.fast ? std::make_tuple(0, 0, 0)
                  : std::make_tuple(t.nb, t.pixel_lanes, t.threads);
  });
  m.def("bn_stage", &bn_stage, py::arg("family"), py::arg("x"),
        py::arg("other"), py::arg("out"), py::arg("mask"), py::arg("ws"),
        py::arg("p"), py::arg("relu"), py::arg("y") = py::none());
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
  m.def("conv_mfma", &conv_mfma, py::arg("x"), py::arg("wk"), py::arg("Cout"),
        py::arg("fh"), py::arg("fw"), py::arg("S"), py::arg("P"), py::arg("D"),
        py::arg("OH"), py::arg("OW"), py::arg("fd") = 1,
        py::arg("out_f32") = false);
  m.def("conv3x3_halo_plan", &conv3x3_halo_plan, py::arg("N"), py::arg("H"),
        py::arg("W"), py::arg("Cin"), py::arg("Cout"), py::arg("fh") = 3,
        py::arg("fw") = 3, py::arg("S") = 1, py::arg("P") = 1,
        py::arg("D") = 1, py::arg("OH") = -1, py::arg("OW") = -1,
        py::arg("fd") = 1, py::arg("out_f32") = false);
  m.def("conv_mfma_stats", &conv_mfma_stats, py::arg("x"), py::arg("wk"),
        py::arg("Cout"), py::arg("fh"), py::arg("fw"), py::arg("S"),
        py::arg("P"), py::arg("D"), py::arg("OH"), py::arg("OW"),
        py::arg("fd") = 1, py::arg("out_f32") = false);
  m.def("gemm_bt_stats", &gemm_bt_stats, py::arg("a"), py::arg("b"));
  m.def("bn_fwd_train_pre", &bn_fwd_train_pre);
  m.def("bn_dual_fwd_train_pre", &bn_dual_fwd_train_pre);
  m.def("bn_batch_stats", &bn_batch_stats);
  m.def("conv_mfma_acc", &conv_mfma_acc, py::arg("x"), py::arg("wk"),
        py::arg("out"), py::arg("fh"), py::arg("fw"), py::arg("S"),
        py::arg("P"), py::arg("D"));
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
  // does gemm_bt_gate take A[M,K] @ B[N,K]^T? (not N % 8 != 0, not a shape
  // on the 256^2 kernel: the caller keeps gemm_bt_acc there)
  m.def("gemm_bt_gate_eligible", [](long M, long N, long K) {
    return M > 0 && M <= INT_MAX && N > 0 && N <= INT_MAX && K > 0 &&
           K <= INT_MAX && tfosr_gemm_bt_gate_eligible((int)M, (int)N, (int)K);
  });
  // dx = A @ B^T + gate(dy, mask): gemm_bt_acc on a c that holds dy where the
  // ReLU bitmask (one byte per 8 elements, as bn_fwd_train returns it) is set
  // and +0 elsewhere, bit for bit, without that tensor: dy and mask are only
  // read, dx is a fresh [M, N] tensor.
  m.def("gemm_bt_gate", [](at::Tensor a, at::Tensor b, at::Tensor dy,
                           at::Tensor mask) {
    TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && dy.dim() == 2,
                "gemm_bt_gate: A[M,K], B[N,K], dy[M,N] must be 2-D");
    TORCH_CHECK(a.is_cuda(), "gemm_bt_gate: a must be a GPU tensor");
    TORCH_CHECK(b.device() == a.device() && dy.device() == a.device() &&
                    mask.device() == a.device(),
                "gemm_bt_gate: b, dy and mask must be on ", a.device());
    TORCH_CHECK(a.is_contiguous() && b.is_contiguous() && dy.is_contiguous() &&
                    mask.is_contiguous(),
                "gemm_bt_gate: a, b, dy and mask must be contiguous");
    TORCH_CHECK(a.scalar_type() == at::kBFloat16 &&
                    b.scalar_type() == at::kBFloat16 &&
                    dy.scalar_type() == at::kBFloat16,
                "gemm_bt_gate: a, b and dy must be bfloat16");
    long M = a.size(0), K = a.size(1), Nn = b.size(0);
    TORCH_CHECK(b.size(1) == K && dy.size(0) == M && dy.size(1) == Nn,
                "gemm_bt_gate: A[M,K], B[N,K], dy[M,N]");
    TORCH_CHECK(K % 32 == 0, "gemm_bt_gate: K must be a multiple of 32");
    TORCH_CHECK(Nn % 8 == 0, "gemm_bt_gate: N must be a multiple of 8, one "
                "mask byte per 8 elements of a row");
    TORCH_CHECK(mask.scalar_type() == at::kByte && mask.numel() == M * Nn / 8,
                "gemm_bt_gate: mask must be uint8 with M * N / 8 elements");
    TORCH_CHECK(M > 0 && M <= INT_MAX && Nn <= INT_MAX && K <= INT_MAX &&
                    tfosr_gemm_bt_gate_eligible((int)M, (int)Nn, (int)K),
                "gemm_bt_gate: no gating epilogue for M ", M, ", N ", Nn,
                ", K ", K, " (gemm_bt_gate_eligible)");
    auto dx = at::empty({M, Nn}, dy.options());
    tfosr_gemm_bt_gate(a.data_ptr(), b.data_ptr(), dy.data_ptr(),
                       mask.data_ptr<unsigned char>(), dx.data_ptr(), (int)M,
                       (int)Nn, (int)K, cur_stream());
    return dx;
  });
  m.def("conv_wrw2", &conv_wrw2, py::arg("dy"), py::arg("x"), py::arg("R"),
        py::arg("S_f"), py::arg("stride"), py::arg("P"), py::arg("fd") = 1);
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
  m.def("conv_par", &conv_par, py::arg("x"), py::arg("wk"), py::arg("out"),
        py::arg("taps_r"), py::arg("taps_s"), py::arg("P"), py::arg("accum"));
  m.def("conv_stem", &conv_stem, py::arg("x4"), py::arg("w224"),
        py::arg("Cout"));
  m.def("conv_stem_wrw", &conv_stem_wrw, py::arg("dy"), py::arg("x4"));
  m.def("conv_wrw", &conv_wrw, py::arg("dy"), py::arg("x"), py::arg("R"),
        py::arg("S"), py::arg("P"));
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

  m.def("convt_head_fwd", &convt_head_fwd, py::arg("x"), py::arg("w"),
        py::arg("bias") = py::none());
  m.def("convt_head_dgrad", &convt_head_dgrad, py::arg("dy"), py::arg("w"),
        py::arg("H"), py::arg("W"));
  m.def("convt_head_wrw", &convt_head_wrw, py::arg("dy"), py::arg("x"));
  m.def("convt_head_info", []() {
    int block, max_grid, fwd_tile, dg_h, dg_w, persist_kb, kstep, min_pix,
        max_blocks, fin_lanes;
    tfosr_convt_head_info(&block, &max_grid, &fwd_tile, &dg_h, &dg_w,
                          &persist_kb, &kstep, &min_pix, &max_blocks,
                          &fin_lanes);
    py::dict d;
    d["block"] = block;
    d["max_grid"] = max_grid;
    d["fwd_tile"] = fwd_tile;
    d["dgrad_tile_h"] = dg_h;
    d["dgrad_tile_w"] = dg_w;
    d["w_persist_kb"] = persist_kb;
    d["wrw_kstep"] = kstep;
    d["wrw_min_pix"] = min_pix;
    d["wrw_max_blocks"] = max_blocks;
    d["fin_lanes"] = fin_lanes;
    return d;
  });
  m.def("convt_head_wrw_plan", [](long M, long Cin, long Cout) {
    TORCH_CHECK(M > 0 && Cin > 0 && Cout > 0, "convt_head_wrw_plan: M, Cin "
                "and Cout must be positive");
    int nblk;
    long slab;
    tfosr_convt_head_wrw_plan(M, (int)Cin, (int)Cout, &nblk, &slab);
    py::dict d;
    d["nblk"] = nblk;
    d["slab"] = slab;
    return d;
  }, py::arg("M"), py::arg("Cin"), py::arg("Cout"));

  m.def("convt_wrw", &convt_wrw, py::arg("dy"), py::arg("x"));
  m.def("convt_wrw_plan", &convt_wrw_plan, py::arg("N"), py::arg("H"),
        py::arg("W"), py::arg("Cin"), py::arg("Cout"));

  m.def("pwconv_fwd", &pwconv_fwd, py::arg("x"), py::arg("w"));
  m.def("pwconv_dgrad", &pwconv_dgrad, py::arg("dy"), py::arg("w"));
  m.def("pwconv_info", []() {
    int tile_m, max_grid, max_c;
    tfosr_pwconv_info(&tile_m, &max_grid, &max_c);
    py::dict d;
    d["tile_m"] = tile_m;
    d["max_grid"] = max_grid;
    d["max_channels"] = max_c;
    return d;
  });
  // M pixels, Ci contracted (fwd: Cin, dgrad: Cout), Co produced; tile_m is
  // this shape's own M tile.
  m.def("pwconv_plan", [](long M, long Ci, long Co) {
    TORCH_CHECK(M > 0 && M <= INT_MAX, "pwconv_plan: M must be in [1, ",
                INT_MAX, "]");
    pw_check_channels("pwconv_plan", "Ci", Ci);
    pw_check_channels("pwconv_plan", "Co", Co);
    const PwPlan p = pw_plan(M, Ci, Co);
    py::dict d;
    d["tile_m"] = p.tile_m;
    d["m_tiles"] = p.m_tiles;
    d["panels"] = p.panels;
    d["grid"] = p.grid;
    d["lds_bytes"] = p.lds_bytes;
    return d;
  }, py::arg("M"), py::arg("Ci"), py::arg("Co"));

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
