// Load-time ops of the pretrained / cross-grid checkpoint path (timm checkpoint_filter_fn):
//   * ivit_pos_resample: F.interpolate(mode='bicubic', antialias=True, align_corners=False) of the
//     patch part of pos_embed, channels last ([h, w, D] is pos_embed[0, prefix:] as it lies in
//     memory). Separable: a width pass into an f64 intermediate, then a height pass; both are the
//     same 1-D kernel over a [outer, n, inner] view with `inner` contiguous (D, then ow * D), one
//     thread per output element, consecutive threads along `inner` (coalesced, any D). Weights and
//     sums in f64: the only rounding of the result is the final one to f32. A gather: no atomics.
//   * ivit_adapt_input_conv: timm adapt_input_conv (3-channel patch weights for C input channels).
// Neither is on a per-step path: they run once per load, a few MB at most.
#include "ivit_common.h"

namespace {

// Keys cubic convolution kernel, a = -0.5 (ATen's bicubic and its antialias filter)
IVIT_DEV double keys_cubic(double x) {
  const double a = -0.5;
  x = fabs(x);
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
  if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
  return 0.0;
}

// dst[o][i][r] = sum_{j in [xmin, xmax)} w_j src[o][j][r],  w_j = k((j - c + 0.5) inv) / sum_j k(..)
// (the formula of ivit.h). The tap count xmax - xmin grows with the down-sampling factor, so the
// weights are evaluated twice (their sum, then the weighted sum) instead of being kept in registers.
template <typename S, typename O>
__global__ __launch_bounds__(256) void resample_axis_kernel(const S* __restrict__ src, long outer, int n_in,
                                                            int n_out, long inner, O* __restrict__ dst) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= outer * n_out * inner) return;
  const long r = idx % inner;
  const int i = (int)((idx / inner) % n_out);
  const long o = idx / (inner * n_out);
  const double scale = (double)n_in / (double)n_out;
  const double support = scale >= 1.0 ? 2.0 * scale : 2.0;
  const double inv = scale >= 1.0 ? 1.0 / scale : 1.0;
  const double c = scale * ((double)i + 0.5);
  int xmin = (int)(c - support + 0.5), xmax = (int)(c + support + 0.5);
  xmin = xmin < 0 ? 0 : xmin;
  xmax = xmax > n_in ? n_in : xmax;
  double total = 0.0;
  for (int j = xmin; j < xmax; ++j) total += keys_cubic(((double)j - c + 0.5) * inv);
  const S* s = src + o * n_in * inner + r;
  double acc = 0.0;
  for (int j = xmin; j < xmax; ++j)
    acc += (keys_cubic(((double)j - c + 0.5) * inv) / total) * (double)s[(long)j * inner];
  dst[idx] = (O)acc;
}

// out[o][c][k] from in[o][I][k], k over the kh * kw taps: mode 0 copy, 1 sum of the 3 input channels,
// 2 in[o][c mod 3][k] * s (s = (float)(3.0 / C))
__global__ __launch_bounds__(256) void adapt_conv_kernel(const float* __restrict__ in, long O, int I, int C, long K,
                                                         int mode, float s, float* __restrict__ out) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= O * C * K) return;
  const long k = idx % K, o = idx / (K * C);
  const int c = (int)((idx / K) % C);
  const float* w = in + o * I * K + k;
  if (mode == 0) out[idx] = w[(long)c * K];
  else if (mode == 1) out[idx] = (w[0] + w[K]) + w[2 * K];
  else out[idx] = w[(long)(c % 3) * K] * s;
}

const long RS_MAX = 1L << 30;  // per-dimension bound: every index above stays far inside a long

}  // namespace

extern "C" long ivit_pos_resample_workspace(long h, long w, long D, long oh, long ow) {
  if (h <= 0 || w <= 0 || D <= 0 || oh <= 0 || ow <= 0) return 0;
  if (h > RS_MAX || w > RS_MAX || D > RS_MAX || oh > RS_MAX || ow > RS_MAX) return 0;
  return h * ow * D * (long)sizeof(double);
}

extern "C" int ivit_pos_resample(const float* src, long h, long w, long D, float* dst, long oh, long ow, void* work,
                                 long work_bytes, void* stream) {
  IVIT_CHECK_ARG(h > 0 && w > 0 && D > 0 && oh > 0 && ow > 0,
                 "ivit_pos_resample: non-positive size (h %ld, w %ld, D %ld, oh %ld, ow %ld)", h, w, D, oh, ow);
  IVIT_CHECK_ARG(h <= RS_MAX && w <= RS_MAX && D <= RS_MAX && oh <= RS_MAX && ow <= RS_MAX,
                 "ivit_pos_resample: size above 2^30");
  IVIT_CHECK_ARG(src && dst, "ivit_pos_resample: null src / dst");
  const long need = ivit_pos_resample_workspace(h, w, D, oh, ow);
  const long n1 = h * ow * D, n2 = oh * ow * D;
  IVIT_CHECK_ARG(n1 / 256 < (1L << 31) - 1 && n2 / 256 < (1L << 31) - 1, "ivit_pos_resample: too many elements");
  IVIT_CHECK_ARG(work && ((uintptr_t)work & 7) == 0, "ivit_pos_resample: null or misaligned (8 B) workspace");
  IVIT_CHECK_ARG(work_bytes >= need, "ivit_pos_resample: workspace of %ld bytes, %ld needed", work_bytes, need);
  hipStream_t st = ivit_stream(stream);
  double* tmp = (double*)work;  // [h, ow, D]
  hipLaunchKernelGGL((resample_axis_kernel<float, double>), dim3(ivit_cdiv(n1, 256)), dim3(256), 0, st, src, h, (int)w,
                     (int)ow, D, tmp);
  IVIT_LAUNCH_CHECK();
  hipLaunchKernelGGL((resample_axis_kernel<double, float>), dim3(ivit_cdiv(n2, 256)), dim3(256), 0, st,
                     (const double*)tmp, 1L, (int)h, (int)oh, ow * D, dst);
  IVIT_LAUNCH_CHECK();
  return 0;
}

extern "C" int ivit_adapt_input_conv(const float* w_in, long O, long I, long kh, long kw, float* w_out, long C,
                                     void* stream) {
  IVIT_CHECK_ARG(O > 0 && I > 0 && kh > 0 && kw > 0 && C > 0,
                 "ivit_adapt_input_conv: non-positive size (O %ld, I %ld, kh %ld, kw %ld, C %ld)", O, I, kh, kw, C);
  IVIT_CHECK_ARG(O <= RS_MAX && I <= RS_MAX && C <= RS_MAX && kh * kw <= RS_MAX && kh <= RS_MAX && kw <= RS_MAX,
                 "ivit_adapt_input_conv: size above 2^30");
  IVIT_CHECK_ARG(C == I || I == 3,
                 "ivit_adapt_input_conv: %ld input channels into %ld: only 3-channel weights are adapted "
                 "(timm adapt_input_conv: NotImplementedError)", I, C);
  IVIT_CHECK_ARG(w_in && w_out, "ivit_adapt_input_conv: null weight pointer");
  const long K = kh * kw, total = O * C * K;
  IVIT_CHECK_ARG(total / 256 < (1L << 31) - 1, "ivit_adapt_input_conv: too many elements");
  const int mode = C == I ? 0 : (C == 1 ? 1 : 2);
  hipLaunchKernelGGL(adapt_conv_kernel, dim3(ivit_cdiv(total, 256)), dim3(256), 0, ivit_stream(stream), w_in, O, (int)I,
                     (int)C, K, mode, (float)(3.0 / (double)C), w_out);
  IVIT_LAUNCH_CHECK();
  return 0;
}
