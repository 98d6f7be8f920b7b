// Attention probabilities of chosen query rows (ivit_attn_rows): for request r = (sample, token),
// out[r, h, :] = softmax_j(q . k_j / sqrt(Dh)) over all N keys of that sample and head, or the mean
// of those rows over the heads. The forward kernels never hold these rows (the bf16 attention is
// flash-style); this is the analysis path beside them and shares nothing with them but the qkv layout.
//
// Launch shape: one 512-thread workgroup per (request, head), or per request when the heads are
// averaged (it then walks the heads in order, so the mean is a fixed-order sum and needs no
// atomics). A wave takes 64 consecutive keys at a time; eight lanes share a K row, each lane reading
// its own 8 of the row's 64 elements (16 B in bf16), so one wave load covers eight whole 128-byte
// rows instead of touching 64 different ones, and a lane only keeps its 8 elements of q. The eight
// partial dot products a lane holds after eight such loads are summed across the eight lanes by a
// transposing butterfly (7 shuffles: lane c of a group ends up with the whole dot product of the
// group's row c), so every lane owns exactly one of the 64 keys. A head is two sweeps over its keys:
//   1. the scores, with a running (max, sum of exp2) per lane; the workgroup combines them (wave
//      butterfly, then the waves' values in wave order) into the row's max M and sum L;
//   2. the same lane stores exp2(u - M) / L for the same keys.
// Between the sweeps the scores of the first `lds_keys` keys wait in LDS (the launcher sizes it:
// min(N rounded up to a tile, AR_LDS_KEYS), 60 KB at most, below the 64 KB a launch may ask for
// without opting in); the keys past that are not stored anywhere, sweep 2 recomputes their dot
// products (N = 18 001: the last 2641 keys), so N is unbounded and nothing is sized by assumption.
// Key j always belongs to the same lane: it reads back the LDS word it wrote itself (no barrier),
// and in the head-mean form `out[r, j]` is only ever touched by one thread.
#include <limits.h>

#include "ivit_common.h"

namespace {

constexpr int AR_THREADS = 512;
constexpr int AR_WAVES = AR_THREADS / 64;
constexpr int AR_DH = 64;
constexpr int AR_LDS_KEYS = 15360;  // scores kept in LDS between the sweeps: 240 tiles, 60 KB

// 8 consecutive elements as f32 by whole 16-byte loads: every address here is qkv (16-byte aligned,
// checked by the entry point) plus a multiple of 8 elements
IVIT_DEV void ld8(const bf16* p, float (&x)[8]) {
  Pack8 v;
  v.u = *(const uint4*)p;
#pragma unroll
  for (int k = 0; k < 8; ++k) x[k] = (float)v.h[k];
}
IVIT_DEV void ld8(const float* p, float (&x)[8]) {
  const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
  x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
}

// One step of the transposing butterfly: lanes l and l ^ W exchange halves of their n partial sums;
// the lane with bit W clear keeps (and completes) the first n / 2, the other the last n / 2.
template <int W, int n>
IVIT_DEV void fold(float (&p)[8], bool hi) {
#pragma unroll
  for (int i = 0; i < n / 2; ++i) {
    const float keep = hi ? p[i + n / 2] : p[i], send = hi ? p[i] : p[i + n / 2];
    p[i] = keep + __shfl_xor(send, W, 64);
  }
}

// The scaled score of this lane's key of the 64-key tile at j0. Lane = (grp, sub) = (lane / 8,
// lane % 8): load i reads elements [8 sub, 8 sub + 8) of row j0 + 8 i + grp; after the butterfly lane
// (grp, sub) holds the dot product of row j0 + 8 sub + grp. Rows >= N are not read (their lanes
// get 0 and are ignored by the caller).
template <typename T>
IVIT_DEV float tile_score(const float (&q8)[8], const T* __restrict__ kp, long ld, int j0, int N, int grp, int sub,
                          float c2) {
  float x[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int j = j0 + 8 * i + grp;
    if (j < N) {
      ld8(kp + (long)j * ld + 8 * sub, x[i]);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) x[i][k] = 0.f;
    }
  }
  float p[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    float a = q8[0] * x[i][0];
#pragma unroll
    for (int k = 1; k < 8; ++k) a = fmaf(q8[k], x[i][k], a);
    p[i] = a;
  }
  fold<4, 8>(p, (sub & 4) != 0);
  fold<2, 4>(p, (sub & 2) != 0);
  fold<1, 2>(p, (sub & 1) != 0);
  return p[0] * c2;
}

// c2: the factor that takes a raw dot product to the base-2 exponent: log2(e)/sqrt(Dh), or 1 when the
// Q block already carries it (q_prescaled). head_mean = 0: grid.y = H, one head per workgroup, out
// [R, H, N]; head_mean = 1: grid.y = 1, the workgroup walks all H heads, out [R, N].
template <typename T>
__global__ __launch_bounds__(AR_THREADS) void attn_rows_kernel(const T* __restrict__ qkv, int B, int N, int H,
                                                               float c2, const int* __restrict__ sample,
                                                               const int* __restrict__ token,
                                                               int head_mean, int lds_keys,
                                                               float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float sc[];  // [lds_keys], a multiple of 64
  const int r = blockIdx.x, tid = threadIdx.x;
  const int s = sample[r], t = token[r];
  const bool mean = head_mean != 0;
  const int h0 = mean ? 0 : blockIdx.y, heads_per_wg = mean ? H : 1;
  float* orow = mean ? out + (long)r * N : out + ((long)r * H + h0) * N;
  if (s < 0 || s >= B || t < 0 || t >= N) {  // a bad request: a zero row, and qkv is not touched
    for (int j = tid; j < N; j += AR_THREADS) orow[j] = 0.f;
    return;
  }
  const long ld = 3L * H * AR_DH;  // elements per token row
  const T* base = qkv + (long)s * N * ld;
  const float inv_heads = 1.0f / (float)heads_per_wg;
  __shared__ float red_m[AR_WAVES], red_l[AR_WAVES];
  const int wave = tid >> 6, lane = tid & 63, grp = lane >> 3, sub = lane & 7;
  const int mine = 8 * sub + grp;  // this lane's key inside a 64-key tile

  for (int hh = 0; hh < heads_per_wg; ++hh) {
    const int h = h0 + hh;
    float q8[8];
    ld8(base + (long)t * ld + (long)h * AR_DH + 8 * sub, q8);
    const T* kp = base + (long)(H + h) * AR_DH;  // K of head h: element (H + h) * Dh of a token row

    // sweep 1: this lane's running max and sum of exp2(u - max)
    float m = -INFINITY, l = 0.f;
    for (int j0 = wave * 64; j0 < N; j0 += AR_THREADS) {  // wave-uniform: the shuffles see all 64 lanes
      const float u = tile_score(q8, kp, ld, j0, N, grp, sub, c2);
      if (j0 < lds_keys) sc[j0 + mine] = u;  // whole tiles: j0 + 63 < lds_keys
      if (j0 + mine < N) {
        const float mn = fmaxf(m, u);
        l = l * fast_exp2(m - mn) + fast_exp2(u - mn);  // m = -inf: 0 * exp2(-inf) = 0
        m = mn;
      }
    }
    // the row's max: butterfly inside the wave, then the waves in order
    const float wm = wave_max(m);
    if (hh > 0) __syncthreads();  // the previous head's reads of red_m / red_l are done
    if (lane == 0) red_m[wave] = wm;
    __syncthreads();
    float M = red_m[0];
#pragma unroll
    for (int w = 1; w < AR_WAVES; ++w) M = fmaxf(M, red_m[w]);
    // N >= 1, so M is finite unless the inputs are not; a lane without keys adds 0
    const float wl = wave_sum(m == -INFINITY ? 0.f : l * fast_exp2(m - M));
    if (lane == 0) red_l[wave] = wl;
    __syncthreads();
    float L = red_l[0];
#pragma unroll
    for (int w = 1; w < AR_WAVES; ++w) L += red_l[w];
    const float scale = (mean ? inv_heads : 1.0f) / L;

    // sweep 2: the probabilities (the same lane owns the same keys as in sweep 1)
    for (int j0 = wave * 64; j0 < N; j0 += AR_THREADS) {
      const float u = j0 < lds_keys ? sc[j0 + mine] : tile_score(q8, kp, ld, j0, N, grp, sub, c2);
      const int j = j0 + mine;
      if (j < N) {
        const float p = fast_exp2(u - M) * scale;
        orow[j] = (mean && hh > 0) ? orow[j] + p : p;
      }
    }
  }
}

}  // namespace

extern "C" int ivit_attn_rows(int dtype, const void* qkv, long B, long N, long H, long Dh, int q_prescaled,
                              const int* sample, const int* token, long R, int head_mean, float* out,
                              void* stream) {
  IVIT_CHECK_ARG(Dh == 64, "ivit_attn_rows: head dim must be 64 (got %ld)", Dh);
  IVIT_CHECK_ARG(dtype == IVIT_F32 || dtype == IVIT_BF16, "ivit_attn_rows: unknown dtype %d", dtype);
  IVIT_CHECK_ARG(!(q_prescaled && dtype != IVIT_BF16), "ivit_attn_rows: q_prescaled needs IVIT_BF16 qkv");
  IVIT_CHECK_ARG(B >= 0 && N >= 0 && H >= 0 && R >= 0, "ivit_attn_rows: negative size (B=%ld N=%ld H=%ld R=%ld)", B, N,
                 H, R);
  IVIT_CHECK_ARG(B <= INT_MAX && N <= INT_MAX && R <= INT_MAX && H <= 65535,
                 "ivit_attn_rows: size out of range (B=%ld N=%ld H=%ld R=%ld)", B, N, H, R);
  if (R == 0 || N == 0 || H == 0) return 0;  // nothing to write
  IVIT_CHECK_ARG(sample && token && out && (qkv || B == 0), "ivit_attn_rows: null pointer");
  IVIT_CHECK_ARG(hal16(qkv), "ivit_attn_rows: qkv must be 16-byte aligned");
  const float c2 = q_prescaled ? 1.0f : 1.4426950408889634f / 8.0f;  // log2(e) / sqrt(64)
  const dim3 grid((unsigned)R, head_mean ? 1u : (unsigned)H);
  const int hm = head_mean ? 1 : 0;
  const long tiles = (N + 63) / 64;
  const int lds_keys = (int)(tiles * 64 < AR_LDS_KEYS ? tiles * 64 : AR_LDS_KEYS);
  const size_t lds = (size_t)lds_keys * sizeof(float);
  hipStream_t st = ivit_stream(stream);
  if (dtype == IVIT_BF16)
    hipLaunchKernelGGL(attn_rows_kernel<bf16>, grid, dim3(AR_THREADS), lds, st, (const bf16*)qkv, (int)B, (int)N,
                       (int)H, c2, sample, token, hm, lds_keys, out);
  else
    hipLaunchKernelGGL(attn_rows_kernel<float>, grid, dim3(AR_THREADS), lds, st, (const float*)qkv, (int)B, (int)N,
                       (int)H, c2, sample, token, hm, lds_keys, out);
  IVIT_LAUNCH_CHECK();
  return 0;
}
