// Masked-autoencoder pre-training ops (He et al. 2021) around the existing ViT blocks:
//   * ivit_token_select: a row gather with a fill row and an additive row table. One form serves the
//     encoder-side gather of the kept tokens, its backward (the inverse index, -1 = zeros: no memset,
//     no atomics), the decoder-side un-shuffle (fill = mask token, add = position table) and the pick
//     of the masked rows for the prediction head. One float4 per lane, consecutive lanes along the
//     row: a 768-B / 1536-B row is 48 / 96 lanes, so every wave instruction moves whole 16-B pieces
//     of at most three rows.
//   * ivit_token_fill_grad: the mask token's gradient, the column sum of the rows that took the fill.
//     Per-block partials in a fixed order, then colreduce_kernel (ivit_common.h): no float atomics,
//     bitwise repeatable.
//   * ivit_mae_loss_fwd / _bwd: mean squared error of the predicted patches against the raster, the
//     target read out of the raster itself (no patch matrix), optionally per-patch normalised.
//     One workgroup per masked patch; a lane owns 16 B of the pred row (4 f32 / 8 bf16), which is
//     half a patch row or a whole one of the raster (16 / 32 contiguous bytes), so pred streams in
//     full lines and the raster in 32-B (P = 8) or 64-B (P = 16) pieces. The caller orders pidx
//     ascending and xcd_remap gives each XCD a contiguous range of patches, so the neighbours in a
//     grid row, which share the raster's 128-B lines, run together behind one L2.
#include "ivit_common.h"

namespace {

const long MAE_MAX = 1L << 30;  // per-dimension bound

__global__ __launch_bounds__(256) void token_select_kernel(const float4* __restrict__ src, long rows, int Ns, int Nd,
                                                           int D4, const int* __restrict__ idx,
                                                           const float4* __restrict__ fill,
                                                           const float4* __restrict__ add, float4* __restrict__ dst) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * D4) return;
  const long r = i / D4;  // b * Nd + j
  const int c = (int)(i - r * D4);
  const long b = r / Nd;
  const int j = (int)(r - b * Nd);
  const int s = idx[r];
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (s >= 0 && s < Ns) v = src[(b * Ns + s) * D4 + c];
  else if (fill) v = fill[c];
  if (add) {
    const float4 a = add[(long)j * D4 + c];
    v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
  }
  dst[i] = v;
}

// part[blockIdx.x][c] = sum over the block's FG_ROWS rows r with idx[r] outside [0, Ns) of dy[r][c]:
// 64 columns x 4 row phases per workgroup (phase p sums rows p, p + 4, ... in order; the phases are
// then added in order), blockIdx.y picks the 64-column slab.
constexpr int FG_ROWS = 64;
__global__ __launch_bounds__(256) void token_fill_grad_kernel(const float* __restrict__ dy, long rows, int Ns, int D,
                                                              const int* __restrict__ idx, float* __restrict__ part) {
  const int cl = threadIdx.x & 63, ph = threadIdx.x >> 6;
  const int c = blockIdx.y * 64 + cl;
  const long r0 = (long)blockIdx.x * FG_ROWS;
  float s = 0.f;
  for (int k = ph; k < FG_ROWS; k += 4) {
    const long r = r0 + k;
    if (r >= rows) break;
    const int t = idx[r];
    if (t < 0 || t >= Ns) s += dy[r * D + c];
  }
  __shared__ float red[4][64];
  red[ph][cl] = s;
  __syncthreads();
  if (ph == 0) part[(long)blockIdx.x * D + c] = ((red[0][cl] + red[1][cl]) + red[2][cl]) + red[3][cl];
}

// ---------------------------------------------------------------- reconstruction loss
// Sum over the workgroup's 256 threads in a fixed order (xor butterflies inside a wave, then the four
// waves in order); every thread gets the result.
IVIT_DEV float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();  // red may still be read from the previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

template <typename T> struct PredVec;
template <> struct PredVec<float> {
  static constexpr int N = 4;
  static IVIT_DEV void load(const float* p, float (&x)[4]) {
    const float4 a = *(const float4*)p;
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
  }
  static IVIT_DEV void store(float* p, const float (&x)[4]) { *(float4*)p = make_float4(x[0], x[1], x[2], x[3]); }
};
template <> struct PredVec<bf16> {
  static constexpr int N = 8;
  static IVIT_DEV void load(const bf16* p, float (&x)[8]) {
    Pack8 q;
    q.u = *(const uint4*)p;
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = (float)q.h[k];
  }
  static IVIT_DEV void store(bf16* p, const float (&x)[8]) {
    *(uint4*)p = f32x8_to_bf16x8(make_float4(x[0], x[1], x[2], x[3]), make_float4(x[4], x[5], x[6], x[7]));
  }
};

// The NV target values of pred columns col .. col + NV - 1 (NV = 4 or 8 divides P, so they lie in
// one raster row): column (c P + ky) P + kx is img[b][c][gy P + ky][gx P + kx]. `patch` points at
// img[b][0][gy P][gx P].
template <int NV>
IVIT_DEV void load_target(const float* __restrict__ patch, int col, int P, long W, long HW, float (&t)[NV]) {
  const int kx = col % P, ky = (col / P) % P, c = col / (P * P);
  const float* p = patch + (long)c * HW + (long)ky * W + kx;
#pragma unroll
  for (int k = 0; k < NV; k += 4) {
    const float4 a = *(const float4*)(p + k);
    t[k] = a.x; t[k + 1] = a.y; t[k + 2] = a.z; t[k + 3] = a.w;
  }
}

// The patch of masked row r, or null when pidx[r] is no patch of the grid (nothing is read then)
IVIT_DEV const float* patch_of(const float* __restrict__ img, const int* __restrict__ pidx, long r, int Nm, int C,
                               int H, int W, int P) {
  const int gw = W / P, np = (H / P) * gw;
  const int pi = pidx[r];
  if (pi < 0 || pi >= np) return nullptr;
  const long b = r / Nm;
  return img + (b * C * H + (long)(pi / gw) * P) * W + (long)(pi % gw) * P;
}

template <typename T>
__global__ __launch_bounds__(256) void mae_loss_fwd_kernel(const T* __restrict__ pred, const float* __restrict__ img,
                                                           int C, int H, int W, int P, const int* __restrict__ pidx,
                                                           int Nm, int norm_pix, float* __restrict__ patch_loss,
                                                           float* __restrict__ stats) {
  constexpr int NV = PredVec<T>::N;
  __shared__ float red[4];
  const long r = xcd_remap(blockIdx.x, gridDim.x);
  const int L = C * P * P;
  const long HW = (long)H * W;
  const float* patch = patch_of(img, pidx, r, Nm, C, H, W, P);
  if (!patch) {  // an index outside the grid: this patch poisons the loss (finite flag 0), reads nothing
    if (threadIdx.x == 0) {
      patch_loss[r] = __builtin_nanf("");
      stats[2 * r] = 0.f;
      stats[2 * r + 1] = 1.f;
    }
    return;
  }
  float mean = 0.f, rstd = 1.f;
  if (norm_pix) {
    // one pass over the patch (the loss pass below then hits L2): sums of d = t - t0 and d^2 with
    // the shift t0 = the patch's first value (the shifted-data form: a large common level cancels
    // in d, not in the sums), combined in f64; var is torch.var's (n - 1)
    const float t0 = patch[0];
    float s = 0.f, q = 0.f;
    for (int col = threadIdx.x * NV; col < L; col += 256 * NV) {
      float t[NV];
      load_target<NV>(patch, col, P, W, HW, t);
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const float d = t[k] - t0;
        s += d;
        q += d * d;
      }
    }
    const double sd = (double)block_sum(s, red), qd = (double)block_sum(q, red);
    const double var = fmax(qd - sd * sd / (double)L, 0.0) / (double)(L - 1);
    mean = (float)((double)t0 + sd / (double)L);
    rstd = (float)(1.0 / sqrt(var + 1e-6));  // an all-zero patch: mean 0, rstd 1000, target 0
  }
  const T* prow = pred + r * L;
  float acc = 0.f;
  for (int col = threadIdx.x * NV; col < L; col += 256 * NV) {
    float t[NV], p[NV];
    PredVec<T>::load(prow + col, p);
    load_target<NV>(patch, col, P, W, HW, t);
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const float d = p[k] - (t[k] - mean) * rstd;
      acc += d * d;
    }
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) {
    patch_loss[r] = acc / (float)L;
    stats[2 * r] = mean;
    stats[2 * r + 1] = rstd;
  }
}

// Scalar loss: the mean of the n per-patch losses in f64, in a fixed order. Stage 1: block k sums
// patches [k * LR_SPAN, (k + 1) * LR_SPAN) (thread t takes t, t + 256, ...; then an LDS tree) and
// counts the non-finite ones -> part[2k], part[2k + 1]. Stage 2 (one block) adds the partials.
constexpr int LR_SPAN = 2048;
IVIT_DEV double block_sum_f64(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}
__global__ __launch_bounds__(256) void mae_loss_partial_kernel(const float* __restrict__ patch_loss, long n,
                                                               double* __restrict__ part) {
  __shared__ double red[256];
  const long lo = (long)blockIdx.x * LR_SPAN;
  double s = 0.0, bad = 0.0;
  for (int k = threadIdx.x; k < LR_SPAN && lo + k < n; k += 256) {
    const float v = patch_loss[lo + k];
    s += (double)v;
    bad += isfinite(v) ? 0.0 : 1.0;
  }
  s = block_sum_f64(s, red);
  bad = block_sum_f64(bad, red);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = s;
    part[2 * blockIdx.x + 1] = bad;
  }
}
__global__ __launch_bounds__(256) void mae_loss_final_kernel(const double* __restrict__ part, int nb, long n,
                                                             float* __restrict__ loss, float* __restrict__ finite) {
  __shared__ double red[256];
  double s = 0.0, bad = 0.0;
  for (int k = threadIdx.x; k < nb; k += 256) {
    s += part[2 * k];
    bad += part[2 * k + 1];
  }
  s = block_sum_f64(s, red);
  bad = block_sum_f64(bad, red);
  if (threadIdx.x == 0) {
    const float l = (float)(s / (double)n);
    *loss = l;
    *finite = (bad == 0.0 && isfinite(l)) ? 1.f : 0.f;
  }
}

// dpred = gout * 2 (pred - target) / (B Nm L), zeros when the forward's flag is 0.
// inv = 2 / (B Nm L) in f64 from the host; one rounding for the scale, one for the product.
template <typename T>
__global__ __launch_bounds__(256) void mae_loss_bwd_kernel(const T* __restrict__ pred, const float* __restrict__ img,
                                                           int C, int H, int W, int P, const int* __restrict__ pidx,
                                                           int Nm, const float* __restrict__ stats,
                                                           const float* __restrict__ gout,
                                                           const float* __restrict__ finite, double inv,
                                                           T* __restrict__ dpred) {
  constexpr int NV = PredVec<T>::N;
  const long r = xcd_remap(blockIdx.x, gridDim.x);
  const int L = C * P * P;
  const long HW = (long)H * W;
  T* drow = dpred + r * L;
  const float* patch = *finite != 0.f ? patch_of(img, pidx, r, Nm, C, H, W, P) : nullptr;
  if (!patch) {
    float z[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) z[k] = 0.f;
    for (int col = threadIdx.x * NV; col < L; col += 256 * NV) PredVec<T>::store(drow + col, z);
    return;
  }
  const float scale = (float)((double)*gout * inv);
  const float mean = stats[2 * r], rstd = stats[2 * r + 1];
  const T* prow = pred + r * L;
  for (int col = threadIdx.x * NV; col < L; col += 256 * NV) {
    float t[NV], p[NV];
    PredVec<T>::load(prow + col, p);
    load_target<NV>(patch, col, P, W, HW, t);
#pragma unroll
    for (int k = 0; k < NV; ++k) p[k] = (p[k] - (t[k] - mean) * rstd) * scale;
    PredVec<T>::store(drow + col, p);
  }
}

int check_tokens(const char* who, long B, long Ns, long D, long Nd) {
  IVIT_CHECK_ARG(B > 0 && Ns > 0 && D > 0 && Nd > 0, "%s: non-positive size (B %ld, Ns %ld, D %ld, Nd %ld)", who, B, Ns,
                 D, Nd);
  IVIT_CHECK_ARG(B <= MAE_MAX && Ns <= MAE_MAX && D <= MAE_MAX && Nd <= MAE_MAX, "%s: size above 2^30", who);
  IVIT_CHECK_ARG(D % 64 == 0, "%s: D %ld is no multiple of 64", who, D);
  IVIT_CHECK_ARG(B * Nd <= MAE_MAX && B * Ns <= MAE_MAX, "%s: more than 2^30 rows", who);
  return 0;
}

int check_loss(const char* who, const void* pred, int pred_dtype, const float* img, long B, long C, long H, long W,
               long P, const int* pidx, long Nm) {
  IVIT_CHECK_ARG(pred_dtype == IVIT_F32 || pred_dtype == IVIT_BF16, "%s: pred dtype %d is neither f32 nor bf16", who,
                 pred_dtype);
  IVIT_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && Nm > 0, "%s: non-positive size (B %ld, C %ld, H %ld, W %ld, Nm %ld)",
                 who, B, C, H, W, Nm);
  IVIT_CHECK_ARG(P == 8 || P == 16, "%s: patch size %ld (8 or 16)", who, P);
  IVIT_CHECK_ARG(H % P == 0 && W % P == 0, "%s: raster %ld x %ld is no multiple of the patch size %ld", who, H, W, P);
  IVIT_CHECK_ARG(B <= MAE_MAX && C <= MAE_MAX && H <= MAE_MAX && W <= MAE_MAX && Nm <= MAE_MAX, "%s: size above 2^30",
                 who);
  IVIT_CHECK_ARG(C * P * P <= MAE_MAX && H * W <= MAE_MAX && B * Nm <= MAE_MAX, "%s: too many elements", who);
  IVIT_CHECK_ARG(Nm <= (H / P) * (W / P), "%s: %ld masked patches in a grid of %ld", who, Nm, (H / P) * (W / P));
  IVIT_CHECK_ARG(pred && img && pidx, "%s: null pred / img / pidx", who);
  IVIT_CHECK_ARG(hal16(pred) && hal16(img), "%s: pred / img not 16-byte aligned", who);
  return 0;
}

}  // namespace

extern "C" int ivit_token_select(const float* src, long B, long Ns, long D, const int* idx, long Nd,
                                 const float* fill, const float* add, float* dst, void* stream) {
  if (int rc = check_tokens("ivit_token_select", B, Ns, D, Nd)) return rc;
  IVIT_CHECK_ARG(src && idx && dst, "ivit_token_select: null src / idx / dst");
  IVIT_CHECK_ARG(hal16(src) && hal16(dst) && hal16(fill) && hal16(add),
                 "ivit_token_select: src / dst / fill / add not 16-byte aligned");
  const long rows = B * Nd, D4 = D / 4;
  IVIT_CHECK_ARG(rows * D4 / 256 < (1L << 31) - 1, "ivit_token_select: too many elements");
  hipLaunchKernelGGL(token_select_kernel, dim3(ivit_cdiv(rows * D4, 256)), dim3(256), 0, ivit_stream(stream),
                     (const float4*)src, rows, (int)Ns, (int)Nd, (int)D4, idx, (const float4*)fill,
                     (const float4*)add, (float4*)dst);
  IVIT_LAUNCH_CHECK();
  return 0;
}

extern "C" long ivit_token_fill_grad_workspace(long B, long Nd, long D) {
  if (B <= 0 || Nd <= 0 || D <= 0 || B > MAE_MAX || Nd > MAE_MAX || D > MAE_MAX || B * Nd > MAE_MAX) return 0;
  return ((B * Nd + FG_ROWS - 1) / FG_ROWS) * D * (long)sizeof(float);
}

extern "C" int ivit_token_fill_grad(const float* dy, long B, long Nd, long D, const int* idx, long Ns, float* dfill,
                                    int accumulate, void* work, long work_bytes, void* stream) {
  if (int rc = check_tokens("ivit_token_fill_grad", B, Ns, D, Nd)) return rc;
  IVIT_CHECK_ARG(dy && idx && dfill, "ivit_token_fill_grad: null dy / idx / dfill");
  const long need = ivit_token_fill_grad_workspace(B, Nd, D);
  IVIT_CHECK_ARG(work && ((uintptr_t)work & 3) == 0, "ivit_token_fill_grad: null or misaligned (4 B) workspace");
  IVIT_CHECK_ARG(work_bytes >= need, "ivit_token_fill_grad: workspace of %ld bytes, %ld needed", work_bytes, need);
  const long rows = B * Nd;
  const int nb = ivit_cdiv(rows, FG_ROWS);
  hipStream_t st = ivit_stream(stream);
  hipLaunchKernelGGL(token_fill_grad_kernel, dim3(nb, (unsigned)(D / 64)), dim3(256), 0, st, dy, rows, (int)Ns, (int)D,
                     idx, (float*)work);
  IVIT_LAUNCH_CHECK();
  launch_colreduce(st, (const float*)work, nb, D, (int)D, dfill, (int)D, nullptr, accumulate ? 1 : 0);
  IVIT_LAUNCH_CHECK();
  return 0;
}

extern "C" long ivit_mae_loss_workspace(long B, long Nm) {
  if (B <= 0 || Nm <= 0 || B > MAE_MAX || Nm > MAE_MAX || B * Nm > MAE_MAX) return 0;
  return ((B * Nm + LR_SPAN - 1) / LR_SPAN) * 2 * (long)sizeof(double);
}

extern "C" int ivit_mae_loss_fwd(const void* pred, int pred_dtype, const float* img, long B, long C, long H, long W,
                                 long P, const int* pidx, long Nm, int norm_pix, float* patch_loss, float* stats,
                                 float* loss, float* finite, void* work, long work_bytes, void* stream) {
  if (int rc = check_loss("ivit_mae_loss_fwd", pred, pred_dtype, img, B, C, H, W, P, pidx, Nm)) return rc;
  IVIT_CHECK_ARG(patch_loss && stats && loss && finite, "ivit_mae_loss_fwd: null patch_loss / stats / loss / finite");
  const long need = ivit_mae_loss_workspace(B, Nm);
  IVIT_CHECK_ARG(work && ((uintptr_t)work & 7) == 0, "ivit_mae_loss_fwd: null or misaligned (8 B) workspace");
  IVIT_CHECK_ARG(work_bytes >= need, "ivit_mae_loss_fwd: workspace of %ld bytes, %ld needed", work_bytes, need);
  const long n = B * Nm;
  const int nb = ivit_cdiv(n, LR_SPAN);
  hipStream_t st = ivit_stream(stream);
  if (pred_dtype == IVIT_BF16)
    hipLaunchKernelGGL(mae_loss_fwd_kernel<bf16>, dim3((unsigned)n), dim3(256), 0, st, (const bf16*)pred, img, (int)C,
                       (int)H, (int)W, (int)P, pidx, (int)Nm, norm_pix, patch_loss, stats);
  else
    hipLaunchKernelGGL(mae_loss_fwd_kernel<float>, dim3((unsigned)n), dim3(256), 0, st, (const float*)pred, img,
                       (int)C, (int)H, (int)W, (int)P, pidx, (int)Nm, norm_pix, patch_loss, stats);
  IVIT_LAUNCH_CHECK();
  hipLaunchKernelGGL(mae_loss_partial_kernel, dim3(nb), dim3(256), 0, st, (const float*)patch_loss, n, (double*)work);
  IVIT_LAUNCH_CHECK();
  hipLaunchKernelGGL(mae_loss_final_kernel, dim3(1), dim3(256), 0, st, (const double*)work, nb, n, loss, finite);
  IVIT_LAUNCH_CHECK();
  return 0;
}

extern "C" int ivit_mae_loss_bwd(const void* pred, int pred_dtype, const float* img, long B, long C, long H, long W,
                                 long P, const int* pidx, long Nm, const float* stats, const float* gout,
                                 const float* finite, void* dpred, void* stream) {
  if (int rc = check_loss("ivit_mae_loss_bwd", pred, pred_dtype, img, B, C, H, W, P, pidx, Nm)) return rc;
  IVIT_CHECK_ARG(stats && gout && finite && dpred, "ivit_mae_loss_bwd: null stats / gout / finite / dpred");
  IVIT_CHECK_ARG(hal16(dpred), "ivit_mae_loss_bwd: dpred not 16-byte aligned");
  const long n = B * Nm;
  const double inv = 2.0 / ((double)n * (double)(C * P * P));
  hipStream_t st = ivit_stream(stream);
  if (pred_dtype == IVIT_BF16)
    hipLaunchKernelGGL(mae_loss_bwd_kernel<bf16>, dim3((unsigned)n), dim3(256), 0, st, (const bf16*)pred, img, (int)C,
                       (int)H, (int)W, (int)P, pidx, (int)Nm, stats, gout, finite, inv, (bf16*)dpred);
  else
    hipLaunchKernelGGL(mae_loss_bwd_kernel<float>, dim3((unsigned)n), dim3(256), 0, st, (const float*)pred, img,
                       (int)C, (int)H, (int)W, (int)P, pidx, (int)Nm, stats, gout, finite, inv, (float*)dpred);
  IVIT_LAUNCH_CHECK();
  return 0;
}
