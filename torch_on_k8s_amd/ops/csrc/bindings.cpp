// Python bindings for the MI355X-native kernels (torch extension).
//
// The kernels themselves live in pure handwritten HIP files (*.hip); this
// translation unit only does tensor checking, workspace allocation and
// stream plumbing. Stream access uses PyTorch-ROCm's native HIP stream
// API (at::hip::getCurrentHIPStreamMasqueradingAsCUDA — the real symbol
// exported by a ROCm build of ATen) so this TU contains no CUDA-named
// calls for hipify to rewrite.
#include <torch/extension.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <hip/hip_runtime.h>

extern "C" {
hipError_t tok_rmsnorm_fwd(const void* x, const void* w, void* y, float* invr,
                           long nrows, int H, float eps, hipStream_t stream);
int tok_rmsnorm_dw_rsplit(long nrows, int H);
hipError_t tok_rmsnorm_bwd(const void* x, const void* w, const void* dy,
                           const float* invr, void* dx, float* dw_f32,
                           float* dw_ws, long nrows, int H,
                           hipStream_t stream);
hipError_t tok_rmsnorm_res_fwd(const void* x, const void* res, const void* w,
                               void* xr, void* y, float* invr, long nrows,
                               int H, float eps, hipStream_t stream);
hipError_t tok_rmsnorm_res_bwd(const void* xr, const void* w, const void* dy,
                               const void* dxr_in, const float* invr,
                               void* dx, float* dw_f32, float* dw_ws,
                               long nrows, int H, hipStream_t stream);
hipError_t tok_swiglu_fwd(const void* gu, void* out, long rows, int I,
                          hipStream_t stream);
hipError_t tok_swiglu_bwd(const void* dout, const void* gu, void* dgu,
                          long rows, int I, hipStream_t stream);
hipError_t tok_qkv_rope_fwd(const void* qkv, void* q, void* k, void* v,
                            const float* cos_tab, const float* sin_tab,
                            long tokens, int Hq, int Hkv, int D,
                            long S, hipStream_t stream,
                            const int* doc_start);
hipError_t tok_qkv_rope_bwd(const void* dq, const void* dk, const void* dv,
                            void* dqkv, const float* cos_tab,
                            const float* sin_tab, long tokens, int Hq,
                            int Hkv, int D, long S,
                            hipStream_t stream, const int* doc_start);
hipError_t tok_rope(const void* x, void* y, const float* cos_tab,
                    const float* sin_tab, long rows_total, int heads, int D,
                    long S, float sign, hipStream_t stream);
hipError_t tok_adamw(void* p, const void* g, float* m, float* v, long n,
                     float lr, float beta1, float beta2, float eps, float wd,
                     int step, float gscale, const int* step_dev,
                     const float* lr_dev, const float* gscale_dev,
                     hipStream_t stream);
hipError_t tok_wgrad_gemm(const void* dy, const void* x, void* c, long M,
                          long N, long K, int accumulate, int group,
                          int variant, long split, hipStream_t stream);
long tok_wgrad_split(long tiles, long cus);
hipError_t tok_wgrad_cus(int* cus);
int tok_wgrad_default_variant();
int tok_grad_sumsq_max_blocks();
int tok_grad_sumsq_blocks(long n);
hipError_t tok_grad_sumsq(const void* g, long n, float* partials, int nblocks,
                          hipStream_t stream);
hipError_t tok_grad_norm_finalize(const float* partials, long count,
                                  float inv_count, float clip, float* out,
                                  hipStream_t stream);
hipError_t tok_mfma_probe_16x16x32(const void* A, const void* B, float* D,
                                   hipStream_t stream);
hipError_t tok_mfma_probe_32x32x16(const void* A, const void* B, float* D,
                                   hipStream_t stream);
hipError_t tok_attn_fwd(const void* q, const void* k, const void* vt, void* o,
                        float* lse, int B, int S, int Hq, int Hkv, int D,
                        int S_pad, int causal, hipStream_t stream,
                        int variant, const int* doc_start);
hipError_t tok_attn_bwd(const void* q, const void* k, const void* v,
                        const void* o, const void* dout, const void* q_t,
                        const void* k_t, const void* dot_t, const float* lse,
                        float* dsum_ws, float* rc_ws, void* dq, void* dk,
                        void* dv, int B, int S, int Hq, int Hkv, int D,
                        int S_pad, int causal, hipStream_t stream, int split,
                        int dq_variant, const int* doc_start,
                        const int* doc_end);
hipError_t tok_transpose_head(const void* in, void* out, int B, int S, int H,
                              int D, int S_pad, hipStream_t stream);
hipError_t tok_transpose_2d(const void* in, void* out, long R, long C,
                            hipStream_t stream);
hipError_t tok_attn_decode(const void* q, const void* k, const void* v,
                           void* out, int B, int T, const int* T_dev,
                           int Tmax, int Hq, int Hkv, int D,
                           hipStream_t stream);
hipError_t tok_attn_decode_ragged(const void* q, const void* k, const void* v,
                                  const int* lens, void* out, float* ws,
                                  int B, int Tmax, int Hq, int Hkv, int D,
                                  int num_splits, int chunk,
                                  hipStream_t stream);
hipError_t tok_qkv_rope_append(const void* qkv, void* q, void* kcache,
                               void* vcache, const float* cos_tab,
                               const float* sin_tab, const int* pos, int B,
                               int Tmax, int Hq, int Hkv, int D,
                               hipStream_t stream);
int tok_sample_max_vocab();
hipError_t tok_sample_tokens(const void* logits, long row_stride,
                             const float* temperature, const int* top_k,
                             const float* top_p, const long long* seed,
                             const void* counter, int counter_is_64,
                             const float* u_opt, long long* out, int B, int V,
                             hipStream_t stream);
hipError_t tok_layernorm_fwd(const void* x, const void* w, const void* b,
                             void* y, float* mu, float* rstd, long nrows,
                             int H, float eps, hipStream_t stream);
hipError_t tok_layernorm_bwd(const void* x, const void* w, const void* dy,
                             const float* mu, const float* rstd, void* dx,
                             float* dw, float* db, long nrows, int H,
                             hipStream_t stream);
hipError_t tok_ce_fwd(const void* logits, const int* labels, float* loss,
                      float* lse, long rows, int V, hipStream_t stream);
hipError_t tok_ce_bwd(const void* logits, const int* labels, const float* lse,
                      const float* gscale, void* dlogits, long rows, int V,
                      hipStream_t stream);
}

namespace {

#define CHECK_BF16_CUDA(t)                                                    \
  TORCH_CHECK(t.is_cuda(), #t " must be on GPU");                             \
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, #t " must be bf16");          \
  TORCH_CHECK(t.is_contiguous(), #t " must be contiguous")

#define TOK_HIP_OK(expr)                                                      \
  do {                                                                        \
    hipError_t _e = (expr);                                                   \
    TORCH_CHECK(_e == hipSuccess, "HIP kernel launch failed: ",               \
                hipGetErrorString(_e));                                       \
  } while (0)

hipStream_t current_stream() {
  return at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
}

std::vector<at::Tensor> rmsnorm_fwd(at::Tensor x, at::Tensor w, double eps) {
  CHECK_BF16_CUDA(x);
  CHECK_BF16_CUDA(w);
  const long H = x.size(-1);
  TORCH_CHECK(H % 8 == 0, "hidden dim must be a multiple of 8");
  TORCH_CHECK(w.numel() == H, "weight shape mismatch");
  const long nrows = x.numel() / H;
  auto y = at::empty_like(x);
  auto invr = at::empty({nrows}, x.options().dtype(at::kFloat));
  TOK_HIP_OK(tok_rmsnorm_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(),
                             invr.data_ptr<float>(), nrows, (int)H,
                             (float)eps, current_stream()));
  return {y, invr};
}

std::vector<at::Tensor> rmsnorm_bwd(at::Tensor x, at::Tensor w, at::Tensor dy,
                                    at::Tensor invr) {
  CHECK_BF16_CUDA(x);
  CHECK_BF16_CUDA(w);
  CHECK_BF16_CUDA(dy);
  const long H = x.size(-1);
  const long nrows = x.numel() / H;
  auto dx = at::empty_like(x);
  auto dw = at::zeros({H}, x.options().dtype(at::kFloat));
  const int rsplit = tok_rmsnorm_dw_rsplit(nrows, (int)H);
  auto ws = at::empty({(long)rsplit * H}, x.options().dtype(at::kFloat));
  TOK_HIP_OK(tok_rmsnorm_bwd(x.data_ptr(), w.data_ptr(), dy.data_ptr(),
                             invr.data_ptr<float>(), dx.data_ptr(),
                             dw.data_ptr<float>(), ws.data_ptr<float>(),
                             nrows, (int)H, current_stream()));
  return {dx, dw};
}

// The fused residual kernels keep a row in registers, at most 8 vectors of
// 8 per thread of a 256-thread block: wider rows have no kernel.
constexpr long kRmsnormResMaxH = 8 * 256 * 8;

// Fused residual + RMSNorm: (x, res?, w) -> (y, xr, invr)
std::vector<at::Tensor> rmsnorm_res_fwd(at::Tensor x,
                                        c10::optional<at::Tensor> res,
                                        at::Tensor w, double eps) {
  CHECK_BF16_CUDA(x);
  CHECK_BF16_CUDA(w);
  const long H = x.size(-1);
  TORCH_CHECK(H % 8 == 0, "hidden dim must be a multiple of 8");
  TORCH_CHECK(H <= kRmsnormResMaxH, "rmsnorm_res: hidden dim ", H,
              " exceeds ", kRmsnormResMaxH);
  TORCH_CHECK(w.numel() == H, "weight shape mismatch");
  const long nrows = x.numel() / H;
  const void* res_p = nullptr;
  if (res.has_value()) {
    CHECK_BF16_CUDA((*res));
    TORCH_CHECK(res->sizes() == x.sizes(), "residual shape mismatch");
    res_p = res->data_ptr();
  }
  auto xr = at::empty_like(x);
  auto y = at::empty_like(x);
  auto invr = at::empty({nrows}, x.options().dtype(at::kFloat));
  TOK_HIP_OK(tok_rmsnorm_res_fwd(x.data_ptr(), res_p, w.data_ptr(),
                                 xr.data_ptr(), y.data_ptr(),
                                 invr.data_ptr<float>(), nrows, (int)H,
                                 (float)eps, current_stream()));
  return {y, xr, invr};
}

std::vector<at::Tensor> rmsnorm_res_bwd(at::Tensor xr, at::Tensor w,
                                        at::Tensor dy,
                                        c10::optional<at::Tensor> dxr,
                                        at::Tensor invr) {
  CHECK_BF16_CUDA(xr);
  CHECK_BF16_CUDA(dy);
  const long H = xr.size(-1);
  TORCH_CHECK(H % 8 == 0, "hidden dim must be a multiple of 8");
  TORCH_CHECK(H <= kRmsnormResMaxH, "rmsnorm_res: hidden dim ", H,
              " exceeds ", kRmsnormResMaxH);
  const long nrows = xr.numel() / H;
  const void* dxr_p = nullptr;
  if (dxr.has_value()) {
    CHECK_BF16_CUDA((*dxr));
    dxr_p = dxr->data_ptr();
  }
  auto dx = at::empty_like(xr);
  auto dw = at::zeros({H}, xr.options().dtype(at::kFloat));
  const int rsplit = tok_rmsnorm_dw_rsplit(nrows, (int)H);
  auto ws = at::empty({(long)rsplit * H}, xr.options().dtype(at::kFloat));
  TOK_HIP_OK(tok_rmsnorm_res_bwd(xr.data_ptr(), w.data_ptr(), dy.data_ptr(),
                                 dxr_p, invr.data_ptr<float>(), dx.data_ptr(),
                                 dw.data_ptr<float>(), ws.data_ptr<float>(),
                                 nrows, (int)H, current_stream()));
  return {dx, dw};
}

// gu: [rows, 2I] packed gate|up -> out [rows, I] = silu(gate)*up
at::Tensor swiglu_fwd(at::Tensor gu) {
  CHECK_BF16_CUDA(gu);
  const long I2 = gu.size(-1);
  TORCH_CHECK(I2 % 16 == 0, "packed gate_up dim must be a multiple of 16");
  const long I = I2 / 2;
  const long rows = gu.numel() / I2;
  auto sizes = gu.sizes().vec();
  sizes.back() = I;
  auto out = at::empty(sizes, gu.options());
  TOK_HIP_OK(tok_swiglu_fwd(gu.data_ptr(), out.data_ptr(), rows, (int)I,
                            current_stream()));
  return out;
}

at::Tensor swiglu_bwd(at::Tensor dout, at::Tensor gu) {
  CHECK_BF16_CUDA(dout);
  CHECK_BF16_CUDA(gu);
  const long I2 = gu.size(-1);
  const long I = I2 / 2;
  const long rows = gu.numel() / I2;
  TORCH_CHECK(dout.numel() == rows * I, "dout shape mismatch");
  auto dgu = at::empty_like(gu);
  TOK_HIP_OK(tok_swiglu_bwd(dout.data_ptr(), gu.data_ptr(), dgu.data_ptr(),
                            rows, (int)I, current_stream()));
  return dgu;
}

// Optional packed-document bounds: int32 [B, S], contiguous, on the data's
// device. Returns nullptr when absent. The values are never read on the
// host; the kernels clamp them.
static const int* doc_bounds_ptr(const c10::optional<at::Tensor>& t,
                                 const at::Tensor& like, long B, long S,
                                 const char* name) {
  if (!t.has_value()) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->device() == like.device(), name,
              " must be on the same device as the data");
  TORCH_CHECK(t->scalar_type() == at::kInt, name, " must be int32");
  TORCH_CHECK(t->is_contiguous() && t->dim() == 2 && t->size(0) == B &&
                  t->size(1) == S,
              name, " must be a contiguous [B, S] tensor");
  return t->data_ptr<int>();
}

// qkv: [B, S, (Hq+2Hkv)*D] -> roped q [B,S,Hq,D], k [B,S,Hkv,D], v [B,S,Hkv,D]
// doc_start: positions count from each token's document start when given
std::vector<at::Tensor> qkv_rope_fwd(at::Tensor qkv, at::Tensor cos_tab,
                                     at::Tensor sin_tab, long Hq, long Hkv,
                                     long D,
                                     c10::optional<at::Tensor> doc_start) {
  CHECK_BF16_CUDA(qkv);
  TORCH_CHECK(cos_tab.scalar_type() == at::kFloat && cos_tab.is_contiguous());
  TORCH_CHECK(sin_tab.scalar_type() == at::kFloat && sin_tab.is_contiguous());
  TORCH_CHECK(D % 16 == 0, "head dim must be a multiple of 16");
  const long B = qkv.size(0), S = qkv.size(1);
  TORCH_CHECK(qkv.size(2) == (Hq + 2 * Hkv) * D, "packed qkv dim mismatch");
  const long tokens = B * S;
  const long table_rows = cos_tab.numel() / (D / 2);
  TORCH_CHECK(sin_tab.numel() == cos_tab.numel(), "cos/sin shape mismatch");
  TORCH_CHECK(table_rows >= S, "rope table has ", table_rows,
              " rows, sequence needs ", S);
  const int* ds = doc_bounds_ptr(doc_start, qkv, B, S, "doc_start");
  auto q = at::empty({B, S, Hq, D}, qkv.options());
  auto k = at::empty({B, S, Hkv, D}, qkv.options());
  auto v = at::empty({B, S, Hkv, D}, qkv.options());
  TOK_HIP_OK(tok_qkv_rope_fwd(qkv.data_ptr(), q.data_ptr(), k.data_ptr(),
                              v.data_ptr(), cos_tab.data_ptr<float>(),
                              sin_tab.data_ptr<float>(), tokens, (int)Hq,
                              (int)Hkv, (int)D, S, current_stream(), ds));
  return {q, k, v};
}

at::Tensor qkv_rope_bwd(at::Tensor dq, at::Tensor dk, at::Tensor dv,
                        at::Tensor cos_tab, at::Tensor sin_tab,
                        c10::optional<at::Tensor> doc_start) {
  CHECK_BF16_CUDA(dq);
  CHECK_BF16_CUDA(dk);
  CHECK_BF16_CUDA(dv);
  const long B = dq.size(0), S = dq.size(1), Hq = dq.size(2), D = dq.size(3);
  const long Hkv = dk.size(2);
  const long tokens = B * S;
  TORCH_CHECK(cos_tab.scalar_type() == at::kFloat && cos_tab.is_contiguous());
  TORCH_CHECK(sin_tab.scalar_type() == at::kFloat && sin_tab.is_contiguous());
  TORCH_CHECK(sin_tab.numel() == cos_tab.numel(), "cos/sin shape mismatch");
  const long table_rows = cos_tab.numel() / (D / 2);
  TORCH_CHECK(table_rows >= S, "rope table has ", table_rows,
              " rows, sequence needs ", S);
  const int* ds = doc_bounds_ptr(doc_start, dq, B, S, "doc_start");
  auto dqkv = at::empty({B, S, (Hq + 2 * Hkv) * D}, dq.options());
  TOK_HIP_OK(tok_qkv_rope_bwd(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
                              dqkv.data_ptr(), cos_tab.data_ptr<float>(),
                              sin_tab.data_ptr<float>(), tokens, (int)Hq,
                              (int)Hkv, (int)D, S, current_stream(), ds));
  return dqkv;
}

at::Tensor rope(at::Tensor x, at::Tensor cos_tab, at::Tensor sin_tab,
                long heads, double sign) {
  CHECK_BF16_CUDA(x);
  TORCH_CHECK(cos_tab.scalar_type() == at::kFloat && cos_tab.is_contiguous());
  TORCH_CHECK(sin_tab.scalar_type() == at::kFloat && sin_tab.is_contiguous());
  const long D = x.size(-1);
  TORCH_CHECK(D % 16 == 0, "head dim must be a multiple of 16");
  const long rows_total = x.numel() / D;
  const long table_rows = cos_tab.numel() / (D / 2);
  TORCH_CHECK(x.dim() >= 3 && x.size(-2) == heads,
              "rope expects [..., S, heads, D]");
  const long S = x.size(-3);
  TORCH_CHECK(sin_tab.numel() == cos_tab.numel(), "cos/sin shape mismatch");
  TORCH_CHECK(table_rows >= S, "rope table has ", table_rows,
              " rows, sequence needs ", S);
  auto y = at::empty_like(x);
  TOK_HIP_OK(tok_rope(x.data_ptr(), y.data_ptr(), cos_tab.data_ptr<float>(),
                      sin_tab.data_ptr<float>(), rows_total, (int)heads,
                      (int)D, S, (float)sign, current_stream()));
  return y;
}

const float* dev_f32_scalar(const c10::optional<at::Tensor>& t,
                            const char* name) {
  if (!t.has_value()) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat &&
                  t->numel() >= 1,
              name, " must be an fp32 GPU scalar");
  return t->data_ptr<float>();
}

void adamw_(at::Tensor p, at::Tensor g, at::Tensor m, at::Tensor v, double lr,
            double beta1, double beta2, double eps, double wd, long step,
            double gscale, c10::optional<at::Tensor> step_dev,
            c10::optional<at::Tensor> lr_dev,
            c10::optional<at::Tensor> gscale_dev) {
  CHECK_BF16_CUDA(p);
  CHECK_BF16_CUDA(g);
  TORCH_CHECK(m.scalar_type() == at::kFloat && v.scalar_type() == at::kFloat);
  const long n = p.numel();
  TORCH_CHECK(n % 8 == 0, "bucket size must be a multiple of 8");
  TORCH_CHECK(g.numel() == n && m.numel() == n && v.numel() == n);
  const int* sd = nullptr;
  if (step_dev.has_value()) {
    TORCH_CHECK(step_dev->scalar_type() == at::kInt && step_dev->is_cuda());
    sd = step_dev->data_ptr<int>();
  }
  const float* lrd = dev_f32_scalar(lr_dev, "lr_dev");
  const float* gsd = dev_f32_scalar(gscale_dev, "gscale_dev");
  TOK_HIP_OK(tok_adamw(p.data_ptr(), g.data_ptr(), m.data_ptr<float>(),
                       v.data_ptr<float>(), n, (float)lr, (float)beta1,
                       (float)beta2, (float)eps, (float)wd, (int)step,
                       (float)gscale, sd, lrd, gsd, current_stream()));
}

long grad_sumsq_blocks(long n) { return tok_grad_sumsq_blocks(n); }

long grad_sumsq_max_blocks() { return tok_grad_sumsq_max_blocks(); }

// One fp32 partial per block into the caller's workspace; allocates
// nothing and does not sync (runs under hipGraph capture).
void grad_sumsq_(at::Tensor g, at::Tensor partials) {
  CHECK_BF16_CUDA(g);
  TORCH_CHECK(partials.is_cuda() && partials.scalar_type() == at::kFloat &&
                  partials.is_contiguous(),
              "partials must be a contiguous fp32 GPU tensor");
  const long n = g.numel();
  TORCH_CHECK(n % 8 == 0, "bucket size must be a multiple of 8");
  const long nb = partials.numel();
  TORCH_CHECK(nb >= 1 && nb <= tok_grad_sumsq_max_blocks(),
              "partials must hold 1..", tok_grad_sumsq_max_blocks(),
              " slots (use grad_sumsq_blocks(n))");
  TOK_HIP_OK(tok_grad_sumsq(g.data_ptr(), n, partials.data_ptr<float>(),
                            (int)nb, current_stream()));
}

void grad_norm_finalize_(at::Tensor partials, at::Tensor out, double inv_count,
                         double clip) {
  TORCH_CHECK(partials.is_cuda() && partials.scalar_type() == at::kFloat &&
                  partials.is_contiguous(),
              "partials must be a contiguous fp32 GPU tensor");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kFloat &&
                  out.is_contiguous() && out.numel() >= 2,
              "out must be a contiguous fp32 GPU tensor of >= 2 elements");
  TOK_HIP_OK(tok_grad_norm_finalize(partials.data_ptr<float>(),
                                    partials.numel(), (float)inv_count,
                                    (float)clip, out.data_ptr<float>(),
                                    current_stream()));
}

// q: [B,S,Hq,D], k/v: [B,S,Hkv,D] bf16 contiguous -> (o, lse[B,Hq,S] f32)
// variant = 0: the v4 forward kernel (default); 1: the older v3, for A/B
// timing and cross-checks in one process.
// doc_start: optional packed-document bounds (query i sees keys
// doc_start[b, i] .. i); causal variant 0 only.
std::vector<at::Tensor> attn_fwd(at::Tensor q, at::Tensor k, at::Tensor v,
                                 bool causal, int64_t variant,
                                 c10::optional<at::Tensor> doc_start) {
  CHECK_BF16_CUDA(q);
  CHECK_BF16_CUDA(k);
  CHECK_BF16_CUDA(v);
  const int B = q.size(0), S = q.size(1), Hq = q.size(2), D = q.size(3);
  const int Hkv = k.size(2);
  TORCH_CHECK(D == 128 || D == 64, "head_dim must be 64 or 128");
  TORCH_CHECK(Hq % Hkv == 0, "GQA requires Hq % Hkv == 0");
  TORCH_CHECK(k.sizes() == v.sizes() && k.size(0) == B && k.size(1) == S);
  TORCH_CHECK(variant == 0 || variant == 1, "attn_fwd variant must be 0 or 1");
  const int* ds = doc_bounds_ptr(doc_start, q, B, S, "doc_start");
  TORCH_CHECK(!ds || (causal && variant == 0),
              "document bounds need causal=true and attn_fwd variant 0");
  auto o = at::empty_like(q);
  auto lse = at::empty({B, Hq, S}, q.options().dtype(at::kFloat));
  const int S_pad = (S + 63) / 64 * 64;
  auto vt = at::empty({B, Hkv, D, S_pad}, q.options());
  TOK_HIP_OK(tok_transpose_head(v.data_ptr(), vt.data_ptr(), B, S, Hkv, D,
                                S_pad, current_stream()));
  TOK_HIP_OK(tok_attn_fwd(q.data_ptr(), k.data_ptr(), vt.data_ptr(),
                          o.data_ptr(), lse.data_ptr<float>(), B, S, Hq, Hkv,
                          D, S_pad, causal ? 1 : 0, current_stream(),
                          (int)variant, ds));
  return {o, lse};
}

// split = false: fused dK+dV kernel (default); true: the older split
// dV / dK kernels, for A/B timing and cross-checks in one process.
// dq_variant = 1: the 8-wave dQ kernel in XCD-aware block order (default);
// 0: the 4-wave dQ kernel; 2: the 8-wave kernel in plain block order.
std::vector<at::Tensor> attn_bwd(at::Tensor q, at::Tensor k, at::Tensor v,
                                 at::Tensor o, at::Tensor lse, at::Tensor dout,
                                 bool causal, bool split, int64_t dq_variant,
                                 c10::optional<at::Tensor> doc_start,
                                 c10::optional<at::Tensor> doc_end) {
  CHECK_BF16_CUDA(q);
  CHECK_BF16_CUDA(dout);
  const int B = q.size(0), S = q.size(1), Hq = q.size(2), D = q.size(3);
  const int Hkv = k.size(2);
  TORCH_CHECK(dq_variant >= 0 && dq_variant <= 2,
              "attn_bwd dq_variant must be 0, 1 or 2");
  // packed-document bounds: dQ masks by doc_start of its q rows, the fused
  // dK+dV kernel by doc_end of its keys
  const int* ds = doc_bounds_ptr(doc_start, q, B, S, "doc_start");
  const int* de = doc_bounds_ptr(doc_end, q, B, S, "doc_end");
  TORCH_CHECK((ds == nullptr) == (de == nullptr),
              "attn_bwd takes doc_start and doc_end together");
  TORCH_CHECK(!ds || (causal && !split && dq_variant == 1),
              "document bounds need causal=true, split=false, dq_variant=1");
  auto dq = at::empty_like(q);
  auto dk = at::empty_like(k);
  auto dv = at::empty_like(v);
  auto dsum = at::empty({B, Hq, S}, q.options().dtype(at::kFloat));
  const int S_pad = (S + 63) / 64 * 64;
  // start values of the fused kernel's S / dP accumulators, written by
  // the Dsum preprocess next to dsum
  auto rc = at::empty({B, Hq, 2, S_pad}, q.options().dtype(at::kFloat));
  auto qt = at::empty({B, Hq, D, S_pad}, q.options());
  auto kt = at::empty({B, Hkv, D, S_pad}, q.options());
  auto dot = at::empty({B, Hq, D, S_pad}, q.options());
  TOK_HIP_OK(tok_transpose_head(q.data_ptr(), qt.data_ptr(), B, S, Hq, D,
                                S_pad, current_stream()));
  TOK_HIP_OK(tok_transpose_head(k.data_ptr(), kt.data_ptr(), B, S, Hkv, D,
                                S_pad, current_stream()));
  TOK_HIP_OK(tok_transpose_head(dout.data_ptr(), dot.data_ptr(), B, S, Hq, D,
                                S_pad, current_stream()));
  TOK_HIP_OK(tok_attn_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                          o.data_ptr(), dout.data_ptr(), qt.data_ptr(),
                          kt.data_ptr(), dot.data_ptr(),
                          lse.data_ptr<float>(), dsum.data_ptr<float>(),
                          rc.data_ptr<float>(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), B, S,
                          Hq, Hkv, D, S_pad, causal ? 1 : 0, current_stream(),
                          split ? 1 : 0, (int)dq_variant, ds, de));
  return {dq, dk, dv};
}

// q: [B, Hq, D]; kcache/vcache: [B, Tmax, Hkv, D] (first T rows valid)
at::Tensor attn_decode(at::Tensor q, at::Tensor kcache, at::Tensor vcache,
                       long T, c10::optional<at::Tensor> T_dev) {
  CHECK_BF16_CUDA(q);
  CHECK_BF16_CUDA(kcache);
  CHECK_BF16_CUDA(vcache);
  const int B = q.size(0), Hq = q.size(1), D = q.size(2);
  const int Tmax = kcache.size(1), Hkv = kcache.size(2);
  TORCH_CHECK(T_dev.has_value() || (T >= 1 && T <= Tmax));
  TORCH_CHECK(D == 64 || D == 128);
  const int* td = nullptr;
  if (T_dev.has_value()) {
    TORCH_CHECK(T_dev->scalar_type() == at::kInt && T_dev->is_cuda());
    td = T_dev->data_ptr<int>();
  }
  auto out = at::empty_like(q);
  TOK_HIP_OK(tok_attn_decode(q.data_ptr(), kcache.data_ptr(),
                             vcache.data_ptr(), out.data_ptr(), B, (int)T,
                             td, Tmax, Hq, Hkv, D, current_stream()));
  return out;
}

// q: [B, Hq, D]; kcache/vcache: [B, Tmax, Hkv, D]; lens: [B] int32 on the
// device, never read by the host. num_splits and chunk come from
// ops.decode_ragged_splits / ops.decode_ragged_chunk (shapes alone).
at::Tensor attn_decode_ragged(at::Tensor q, at::Tensor kcache,
                              at::Tensor vcache, at::Tensor lens,
                              long num_splits, long chunk) {
  CHECK_BF16_CUDA(q);
  CHECK_BF16_CUDA(kcache);
  CHECK_BF16_CUDA(vcache);
  TORCH_CHECK(q.dim() == 3 && kcache.dim() == 4, "q [B,Hq,D], cache [B,T,Hkv,D]");
  const long B = q.size(0), Hq = q.size(1), D = q.size(2);
  const long Tmax = kcache.size(1), Hkv = kcache.size(2);
  TORCH_CHECK(kcache.sizes() == vcache.sizes() && kcache.size(0) == B &&
                  kcache.size(3) == D, "cache shape mismatch");
  TORCH_CHECK(D == 64 || D == 128, "head_dim must be 64 or 128");
  TORCH_CHECK(Hkv >= 1 && Hq % Hkv == 0, "GQA requires Hq % Hkv == 0");
  const long R = Hq / Hkv;
  TORCH_CHECK(R == 1 || R == 2 || R == 4 || R == 8,
              "attn_decode_ragged: Hq/Hkv must be 1, 2, 4 or 8, got ", R);
  TORCH_CHECK(lens.is_cuda() && lens.scalar_type() == at::kInt &&
                  lens.is_contiguous() && lens.numel() == B,
              "lens must be a contiguous int32 GPU tensor of B elements");
  TORCH_CHECK(Tmax >= 1 && Tmax < (1L << 26), "Tmax out of range");
  TORCH_CHECK(B >= 1 && B <= 65535 && num_splits >= 1 && num_splits <= 1024,
              "grid out of range");
  TORCH_CHECK(chunk >= 1 && num_splits * chunk >= Tmax,
              "num_splits * chunk must cover Tmax");
  auto out = at::empty_like(q);
  at::Tensor ws;
  float* wsp = nullptr;
  if (num_splits > 1) {
    ws = at::empty({B * Hq * num_splits * (D + 2)},
                   q.options().dtype(at::kFloat));
    wsp = ws.data_ptr<float>();
  }
  TOK_HIP_OK(tok_attn_decode_ragged(
      q.data_ptr(), kcache.data_ptr(), vcache.data_ptr(),
      lens.data_ptr<int>(), out.data_ptr(), wsp, (int)B, (int)Tmax, (int)Hq,
      (int)Hkv, (int)D, (int)num_splits, (int)chunk, current_stream()));
  return out;
}

// qkv: [B, (Hq+2Hkv)*D], one new token per sequence; pos: [B] int32 on the
// device. Writes k/v into cache[b, pos[b]] in place and returns roped q.
at::Tensor qkv_rope_append_(at::Tensor qkv, at::Tensor cos_tab,
                            at::Tensor sin_tab, at::Tensor pos,
                            at::Tensor kcache, at::Tensor vcache, long Hq,
                            long Hkv, long D) {
  CHECK_BF16_CUDA(qkv);
  CHECK_BF16_CUDA(kcache);
  CHECK_BF16_CUDA(vcache);
  TORCH_CHECK(cos_tab.is_cuda() && cos_tab.scalar_type() == at::kFloat &&
              cos_tab.is_contiguous());
  TORCH_CHECK(sin_tab.is_cuda() && sin_tab.scalar_type() == at::kFloat &&
              sin_tab.is_contiguous());
  TORCH_CHECK(D % 16 == 0, "head dim must be a multiple of 16");
  TORCH_CHECK(qkv.dim() == 2 && qkv.size(1) == (Hq + 2 * Hkv) * D,
              "packed qkv must be [B, (Hq+2Hkv)*D]");
  const long B = qkv.size(0);
  TORCH_CHECK(kcache.dim() == 4 && kcache.sizes() == vcache.sizes() &&
                  kcache.size(0) == B && kcache.size(2) == Hkv &&
                  kcache.size(3) == D, "cache shape mismatch");
  const long Tmax = kcache.size(1);
  TORCH_CHECK(pos.is_cuda() && pos.scalar_type() == at::kInt &&
                  pos.is_contiguous() && pos.numel() == B,
              "pos must be a contiguous int32 GPU tensor of B elements");
  TORCH_CHECK(sin_tab.numel() == cos_tab.numel(), "cos/sin shape mismatch");
  const long table_rows = cos_tab.numel() / (D / 2);
  TORCH_CHECK(table_rows >= Tmax, "rope table has ", table_rows,
              " rows, cache needs ", Tmax);
  auto q = at::empty({B, Hq, D}, qkv.options());
  TOK_HIP_OK(tok_qkv_rope_append(
      qkv.data_ptr(), q.data_ptr(), kcache.data_ptr(), vcache.data_ptr(),
      cos_tab.data_ptr<float>(), sin_tab.data_ptr<float>(),
      pos.data_ptr<int>(), (int)B, (int)Tmax, (int)Hq, (int)Hkv, (int)D,
      current_stream()));
  return q;
}

// logits: [B, V] bf16, unit stride in V, any row stride. The per-row
// parameters are [B] device tensors that the host never reads; u replaces
// the generator's draw when given. Returns int64 [B].
at::Tensor sample_tokens(at::Tensor logits, at::Tensor temperature,
                         at::Tensor top_k, at::Tensor top_p, at::Tensor seed,
                         at::Tensor counter, c10::optional<at::Tensor> u) {
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == at::kBFloat16 &&
                  logits.dim() == 2,
              "sample_tokens: logits must be a [B, V] bf16 GPU tensor");
  const long B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(B >= 1 && V >= 1 && V <= tok_sample_max_vocab(),
              "sample_tokens: need B >= 1 and 1 <= V <= ",
              tok_sample_max_vocab());
  TORCH_CHECK(logits.stride(1) == 1 || V == 1,
              "sample_tokens: logits must have unit stride in V");
  auto row_ok = [&](const at::Tensor& t, at::ScalarType ty, const char* n) {
    TORCH_CHECK(t.is_cuda() && t.get_device() == logits.get_device() &&
                    t.scalar_type() == ty && t.is_contiguous() &&
                    t.numel() == B,
                "sample_tokens: ", n, " must be a contiguous [B] tensor of ",
                c10::toString(ty), " on the logits' device");
  };
  row_ok(temperature, at::kFloat, "temperature");
  row_ok(top_k, at::kInt, "top_k");
  row_ok(top_p, at::kFloat, "top_p");
  row_ok(seed, at::kLong, "seed");
  const bool c64 = counter.scalar_type() == at::kLong;
  row_ok(counter, c64 ? at::kLong : at::kInt, "counter");
  const float* up = nullptr;
  if (u.has_value()) {
    row_ok(*u, at::kFloat, "u");
    up = u->data_ptr<float>();
  }
  auto out = at::empty({B}, logits.options().dtype(at::kLong));
  TOK_HIP_OK(tok_sample_tokens(
      logits.data_ptr(), B > 1 ? logits.stride(0) : 0,
      temperature.data_ptr<float>(), top_k.data_ptr<int>(),
      top_p.data_ptr<float>(),
      reinterpret_cast<const long long*>(seed.data_ptr<int64_t>()),
      counter.data_ptr(), c64 ? 1 : 0, up,
      reinterpret_cast<long long*>(out.data_ptr<int64_t>()), (int)B, (int)V,
      current_stream()));
  return out;
}

std::vector<at::Tensor> layernorm_fwd(at::Tensor x, at::Tensor w,
                                      at::Tensor b, double eps) {
  CHECK_BF16_CUDA(x);
  CHECK_BF16_CUDA(w);
  CHECK_BF16_CUDA(b);
  const long H = x.size(-1);
  TORCH_CHECK(H % 8 == 0, "hidden dim must be a multiple of 8");
  const long nrows = x.numel() / H;
  auto y = at::empty_like(x);
  auto mu = at::empty({nrows}, x.options().dtype(at::kFloat));
  auto rstd = at::empty({nrows}, x.options().dtype(at::kFloat));
  TOK_HIP_OK(tok_layernorm_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(),
                               y.data_ptr(), mu.data_ptr<float>(),
                               rstd.data_ptr<float>(), nrows, (int)H,
                               (float)eps, current_stream()));
  return {y, mu, rstd};
}

std::vector<at::Tensor> layernorm_bwd(at::Tensor x, at::Tensor w,
                                      at::Tensor dy, at::Tensor mu,
                                      at::Tensor rstd) {
  CHECK_BF16_CUDA(x);
  const long H = x.size(-1);
  const long nrows = x.numel() / H;
  auto dx = at::empty_like(x);
  auto dw = at::zeros({H}, x.options().dtype(at::kFloat));
  auto db = at::zeros({H}, x.options().dtype(at::kFloat));
  TOK_HIP_OK(tok_layernorm_bwd(x.data_ptr(), w.data_ptr(), dy.data_ptr(),
                               mu.data_ptr<float>(), rstd.data_ptr<float>(),
                               dx.data_ptr(), dw.data_ptr<float>(),
                               db.data_ptr<float>(), nrows, (int)H,
                               current_stream()));
  return {dx, dw, db};
}

std::vector<at::Tensor> ce_fwd(at::Tensor logits, at::Tensor labels) {
  CHECK_BF16_CUDA(logits);
  TORCH_CHECK(labels.scalar_type() == at::kInt && labels.is_cuda());
  const long V = logits.size(-1);
  TORCH_CHECK(V % 8 == 0, "vocab must be a multiple of 8");
  const long rows = logits.numel() / V;
  TORCH_CHECK(labels.numel() == rows);
  auto loss = at::empty({rows}, logits.options().dtype(at::kFloat));
  auto lse = at::empty({rows}, logits.options().dtype(at::kFloat));
  TOK_HIP_OK(tok_ce_fwd(logits.data_ptr(), labels.data_ptr<int>(),
                        loss.data_ptr<float>(), lse.data_ptr<float>(), rows,
                        (int)V, current_stream()));
  return {loss, lse};
}

at::Tensor ce_bwd(at::Tensor logits, at::Tensor labels, at::Tensor lse,
                  at::Tensor gscale) {
  CHECK_BF16_CUDA(logits);
  TORCH_CHECK(gscale.scalar_type() == at::kFloat && gscale.is_cuda());
  const long V = logits.size(-1);
  const long rows = logits.numel() / V;
  auto dlogits = at::empty_like(logits);
  TOK_HIP_OK(tok_ce_bwd(logits.data_ptr(), labels.data_ptr<int>(),
                        lse.data_ptr<float>(), gscale.data_ptr<float>(),
                        dlogits.data_ptr(), rows, (int)V, current_stream()));
  return dlogits;
}

at::Tensor mfma_probe(at::Tensor A, at::Tensor B) {
  CHECK_BF16_CUDA(A);
  CHECK_BF16_CUDA(B);
  if (A.size(0) == 16) {
    TORCH_CHECK(A.sizes() == at::IntArrayRef({16, 32}) &&
                B.sizes() == at::IntArrayRef({32, 16}));
    auto D = at::empty({16, 16}, A.options().dtype(at::kFloat));
    TOK_HIP_OK(tok_mfma_probe_16x16x32(A.data_ptr(), B.data_ptr(),
                                       D.data_ptr<float>(), current_stream()));
    return D;
  }
  TORCH_CHECK(A.sizes() == at::IntArrayRef({32, 16}) &&
              B.sizes() == at::IntArrayRef({16, 32}));
  auto D = at::empty({32, 32}, A.options().dtype(at::kFloat));
  TOK_HIP_OK(tok_mfma_probe_32x32x16(A.data_ptr(), B.data_ptr(),
                                     D.data_ptr<float>(), current_stream()));
  return D;
}

}  // namespace

// out[N,K] (+)= dy[M,N]^T x[M,K] by the hand kernel. The caller (ops.
// wgrad_gemm_) has checked the shape rules; this re-checks what would
// otherwise read or write out of bounds. Allocates nothing, does not sync.
// `variant` < 0: the default schedule; `split` < 0: the rule for the device's
// compute units (wgrad_split). Every choice gives the same bits.
void wgrad_gemm_(at::Tensor dy, at::Tensor x, at::Tensor out, bool accumulate,
                 int64_t group, int64_t variant, int64_t split) {
  CHECK_BF16_CUDA(dy);
  CHECK_BF16_CUDA(x);
  CHECK_BF16_CUDA(out);
  TORCH_CHECK(dy.dim() == 2 && x.dim() == 2 && out.dim() == 2,
              "wgrad_gemm_: dy, x and out must be 2-D");
  const long M = dy.size(0), N = dy.size(1), K = x.size(1);
  TORCH_CHECK(x.size(0) == M && out.size(0) == N && out.size(1) == K,
              "wgrad_gemm_: need dy [M,N], x [M,K], out [N,K]");
  TORCH_CHECK(M >= 64 && M % 64 == 0 && N >= 256 && N % 256 == 0 &&
                  K >= 256 && K % 256 == 0,
              "wgrad_gemm_: needs M % 64 == 0 and N, K multiples of 256");
  TORCH_CHECK(((uintptr_t)dy.data_ptr() | (uintptr_t)x.data_ptr() |
               (uintptr_t)out.data_ptr()) % 16 == 0,
              "wgrad_gemm_: pointers must be 16-byte aligned");
  TORCH_CHECK(group >= 1, "wgrad_gemm_: group must be >= 1");
  TORCH_CHECK(variant <= 1, "wgrad_gemm_: variant must be 0, 1 or negative");
  TORCH_CHECK(split <= (N / 256) * (K / 256),
              "wgrad_gemm_: split must not exceed the number of tiles");
  TOK_HIP_OK(tok_wgrad_gemm(dy.data_ptr(), x.data_ptr(), out.data_ptr(), M, N,
                            K, accumulate ? 1 : 0, (int)group,
                            variant < 0 ? -1 : (int)variant,
                            split < 0 ? -1L : (long)split, current_stream()));
}

// The split rule of wgrad_gemm_ for an [N, K] output on `cus` compute units.
int64_t wgrad_split(int64_t N, int64_t K, int64_t cus) {
  return tok_wgrad_split((N / 256) * (K / 256), cus);
}

// Compute units of the current device, as wgrad_gemm_ counts them.
int64_t wgrad_cus() {
  int cus = 0;
  TOK_HIP_OK(tok_wgrad_cus(&cus));
  return cus;
}

int64_t wgrad_default_variant() { return tok_wgrad_default_variant(); }

// out[C,R] = in[R,C]^T, bf16 bit patterns, by weight_transpose_kernel. The
// caller (ops.transpose_2d_) has checked the contract and raises ValueError;
// this re-checks what would otherwise read or write out of bounds. One
// launch on the current stream, no allocation, no sync.
void transpose_2d_(at::Tensor in, at::Tensor out) {
  CHECK_BF16_CUDA(in);
  CHECK_BF16_CUDA(out);
  TORCH_CHECK(in.dim() == 2 && out.dim() == 2 &&
                  out.size(0) == in.size(1) && out.size(1) == in.size(0),
              "transpose_2d_: need in [R,C] and out [C,R]");
  TORCH_CHECK(in.get_device() == out.get_device(),
              "transpose_2d_: in and out must be on one device");
  const long R = in.size(0), C = in.size(1);
  TORCH_CHECK(R >= 8 && C >= 8 && R % 8 == 0 && C % 8 == 0,
              "transpose_2d_: R and C must be multiples of 8");
  const uintptr_t a = (uintptr_t)in.data_ptr(), b = (uintptr_t)out.data_ptr();
  TORCH_CHECK((a | b) % 16 == 0,
              "transpose_2d_: pointers must be 16-byte aligned");
  const uintptr_t bytes = (uintptr_t)R * C * 2;
  TORCH_CHECK(a + bytes <= b || b + bytes <= a,
              "transpose_2d_: in and out must not overlap");
  TOK_HIP_OK(tok_transpose_2d(in.data_ptr(), out.data_ptr(), R, C,
                              current_stream()));
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, mod) {
  mod.def("mfma_probe", &mfma_probe, "MFMA 16x16x32 bf16 layout probe");
  mod.def("attn_fwd", &attn_fwd, "Flash attention forward (bf16, gfx950)",
          py::arg("q"), py::arg("k"), py::arg("v"), py::arg("causal"),
          py::arg("variant") = 0, py::arg("doc_start") = py::none());
  mod.def("attn_bwd", &attn_bwd, "Flash attention backward (bf16, gfx950)",
          py::arg("q"), py::arg("k"), py::arg("v"), py::arg("o"),
          py::arg("lse"), py::arg("dout"), py::arg("causal"),
          py::arg("split") = false, py::arg("dq_variant") = 1,
          py::arg("doc_start") = py::none(), py::arg("doc_end") = py::none());
  mod.def("ce_fwd", &ce_fwd, "Fused cross-entropy forward (bf16, gfx950)");
  mod.def("layernorm_fwd", &layernorm_fwd, "LayerNorm forward (bf16, gfx950)");
  mod.def("attn_decode", &attn_decode,
          "Single-token KV-cache attention decode (bf16, gfx950)",
          py::arg("q"), py::arg("kcache"), py::arg("vcache"), py::arg("T"),
          py::arg("T_dev") = py::none());
  mod.def("attn_decode_ragged", &attn_decode_ragged,
          "Per-sequence-length KV-cache attention decode (bf16, gfx950)",
          py::arg("q"), py::arg("kcache"), py::arg("vcache"), py::arg("lens"),
          py::arg("num_splits"), py::arg("chunk"));
  mod.def("qkv_rope_append_", &qkv_rope_append_,
          "One-token packed-QKV RoPE + KV-cache append (bf16, gfx950)");
  mod.def("sample_tokens", &sample_tokens,
          "Fused temperature / top-k / top-p sampler (bf16, gfx950)",
          py::arg("logits"), py::arg("temperature"), py::arg("top_k"),
          py::arg("top_p"), py::arg("seed"), py::arg("counter"),
          py::arg("u") = py::none());
  mod.def("layernorm_bwd", &layernorm_bwd, "LayerNorm backward (bf16, gfx950)");
  mod.def("ce_bwd", &ce_bwd, "Fused cross-entropy backward (bf16, gfx950)");
  mod.def("rmsnorm_fwd", &rmsnorm_fwd, "RMSNorm forward (bf16, gfx950)");
  mod.def("rmsnorm_bwd", &rmsnorm_bwd, "RMSNorm backward (bf16, gfx950)");
  mod.def("rmsnorm_res_fwd", &rmsnorm_res_fwd,
          "Fused residual-add + RMSNorm forward (bf16, gfx950)",
          py::arg("x"), py::arg("res"), py::arg("w"), py::arg("eps"));
  mod.def("rmsnorm_res_bwd", &rmsnorm_res_bwd,
          "Fused residual-add + RMSNorm backward (bf16, gfx950)",
          py::arg("xr"), py::arg("w"), py::arg("dy"), py::arg("dxr"),
          py::arg("invr"));
  mod.def("swiglu_fwd", &swiglu_fwd,
          "Fused SwiGLU over packed gate_up (bf16, gfx950)");
  mod.def("swiglu_bwd", &swiglu_bwd,
          "Fused SwiGLU backward (bf16, gfx950)");
  mod.def("qkv_rope_fwd", &qkv_rope_fwd,
          "Packed-QKV split + RoPE (bf16, gfx950)", py::arg("qkv"),
          py::arg("cos_tab"), py::arg("sin_tab"), py::arg("Hq"),
          py::arg("Hkv"), py::arg("D"), py::arg("doc_start") = py::none());
  mod.def("qkv_rope_bwd", &qkv_rope_bwd,
          "Packed-QKV gather + inverse RoPE (bf16, gfx950)", py::arg("dq"),
          py::arg("dk"), py::arg("dv"), py::arg("cos_tab"),
          py::arg("sin_tab"), py::arg("doc_start") = py::none());
  mod.def("rope", &rope, "Rotary embedding rotate-half (bf16, gfx950)");
  mod.def("adamw_", &adamw_, "Fused AdamW on a flat bucket (gfx950)",
          py::arg("p"), py::arg("g"), py::arg("m"), py::arg("v"),
          py::arg("lr"), py::arg("beta1"), py::arg("beta2"), py::arg("eps"),
          py::arg("wd"), py::arg("step"), py::arg("gscale"),
          py::arg("step_dev") = py::none(), py::arg("lr_dev") = py::none(),
          py::arg("gscale_dev") = py::none());
  mod.def("grad_sumsq_blocks", &grad_sumsq_blocks,
          "Partial slots grad_sumsq_ needs for a bucket of n elements");
  mod.def("grad_sumsq_max_blocks", &grad_sumsq_max_blocks,
          "Grid cap of grad_sumsq_");
  mod.def("grad_sumsq_", &grad_sumsq_,
          "Per-block sum of squares of a flat bf16 bucket (gfx950)");
  mod.def("grad_norm_finalize_", &grad_norm_finalize_,
          "Sum partials -> {norm, clip-folded grad scale} (gfx950)",
          py::arg("partials"), py::arg("out"), py::arg("inv_count"),
          py::arg("clip"));
  mod.def("wgrad_gemm_", &wgrad_gemm_,
          "out[N,K] (+)= dy[M,N]^T x[M,K], bf16, fp32 accumulate (gfx950)",
          py::arg("dy"), py::arg("x"), py::arg("out"), py::arg("accumulate"),
          py::arg("group"), py::arg("variant") = -1, py::arg("split") = -1);
  mod.def("wgrad_split", &wgrad_split,
          "Trailing tiles wgrad_gemm_ computes as half blocks",
          py::arg("N"), py::arg("K"), py::arg("cus"));
  mod.def("wgrad_cus", &wgrad_cus, "Compute units of the current device");
  mod.def("wgrad_default_variant", &wgrad_default_variant,
          "Schedule wgrad_gemm_ runs when variant is negative");
  mod.def("transpose_2d_", &transpose_2d_,
          "out[C,R] = in[R,C]^T, bf16 bit patterns (gfx950)",
          py::arg("src"), py::arg("out"));
}
