// Small bandwidth-bound kernels: dtype casts, column-slice copies, the head output split
// (heads.py:18-25,39-43 view/permute + model_vit.py:181-184 reshape) and fused AdamW
// (torch.optim.AdamW as used at train_vit.py:130).
#include "ivit_common.h"

namespace {

IVIT_DEV float ldv(const void* p, int dt, long i) {
  return dt == IVIT_BF16 ? bf2f(((const bf16*)p)[i]) : ((const float*)p)[i];
}
IVIT_DEV void stv(void* p, int dt, long i, float v) {
  if (dt == IVIT_BF16) ((bf16*)p)[i] = f2bf(v);
  else ((float*)p)[i] = v;
}

__global__ void cast_kernel(const void* x, int xdt, void* y, int ydt, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) stv(y, ydt, i, ldv(x, xdt, i));
}

__global__ void add_act_grad_kernel(const void* a, int adt, const void* b, int bdt, const void* pre, int pdt,
                                    const float* rs, long re, void* out, int odt, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float v = ldv(a, adt, i);
  if (b) v += ldv(b, bdt, i);
  if (pre) v *= gelu_erf_grad(ldv(pre, pdt, i));
  if (rs) v *= rs[i / re];
  stv(out, odt, i, v);
}

// 8 elements per thread (n % 8 == 0, row_elems % 8 == 0, 16-B aligned operands): the same per-element
// arithmetic and order as add_act_grad_kernel, 16-B accesses
__global__ __launch_bounds__(256) void add_act_grad8_kernel(const void* a, int adt, const void* b, int bdt,
                                                           const void* pre, int pdt, const float* rs, long re,
                                                           void* out, int odt, long n) {
  const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (i >= n) return;
  float v[8], w[8];
  ld8dt(a, adt, i, v);
  if (b) {
    ld8dt(b, bdt, i, w);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] += w[e];
  }
  if (pre) {
    ld8dt(pre, pdt, i, w);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] *= gelu_erf_grad(w[e]);
  }
  if (rs) {
    const float r = rs[i / re];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] *= r;
  }
  st8dt(out, odt, i, v);
}

// standalone activation modules (nn.GELU exact erf / nn.ReLU) and their input gradients
__global__ void act_fwd_kernel(int act, const void* x, int xdt, void* y, int ydt, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float v = ldv(x, xdt, i);
  stv(y, ydt, i, act == IVIT_ACT_GELU ? gelu_erf(v) : (act == IVIT_ACT_RELU ? (v > 0.f ? v : 0.f) : v));
}
__global__ void act_bwd_kernel(int act, const void* dy, int dydt, const void* x, int xdt, void* dx, int dxdt,
                               long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float g = ldv(dy, dydt, i), v = ldv(x, xdt, i);
  stv(dx, dxdt, i, act == IVIT_ACT_GELU ? g * gelu_erf_grad(v) : (act == IVIT_ACT_RELU ? (v > 0.f ? g : 0.f) : g));
}

__global__ void copy_cols_kernel(const void* src, long lds, void* dst, long ldd, long rows, long cols, int dt) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * cols) return;
  const long r = i / cols, c = i - r * cols;
  stv(dst, dt, r * ldd + c, ldv(src, dt, r * lds + c));
}

// head row m (one BEV cell), anchor a: det channel a*7 + j (j=0 cls, 1..6 box),
// intent channel A*7 + a*K + k.  Flat anchor index = m*A + a  (model_vit.py:183-184).
__global__ void split_heads_kernel(const float* __restrict__ h, long ldh, long M, int A, int K, float* cls,
                                   float* box, float* intent) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // over M*A
  if (i >= M * A) return;
  const long m = i / A;
  const int a = (int)(i - m * A);
  const float* r = h + m * ldh;
  cls[i] = r[a * 7];
#pragma unroll
  for (int j = 0; j < 6; ++j) box[i * 6 + j] = r[a * 7 + 1 + j];
  for (int k = 0; k < K; ++k) intent[i * K + k] = r[A * 7 + a * K + k];
}

__global__ void merge_heads_kernel(const float* dcls, const float* dbox, const float* dint, long M, int A, int K,
                                   void* dh, long ldh, int dt) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // over M*ldh
  if (i >= M * ldh) return;
  const long m = i / ldh;
  const int c = (int)(i - m * ldh);
  float v = 0.f;
  if (c < A * 7) {
    const int a = c / 7, j = c - a * 7;
    const long fa = m * A + a;
    v = j == 0 ? (dcls ? dcls[fa] : 0.f) : (dbox ? dbox[fa * 6 + j - 1] : 0.f);
  } else if (c < A * 7 + A * K) {
    const int cc = c - A * 7, a = cc / K, k = cc - a * K;
    v = dint ? dint[(m * A + a) * K + k] : 0.f;
  }
  stv(dh, dt, i, v);
}

// torch _multi_tensor_adamw (foreach=True, amsgrad=False, maximize=False):
//   p *= 1 - lr*wd ; m = lerp(m, g, 1-b1) ; v = v*b2 + (1-b2) g^2
//   p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
// shadows (optional): per tensor a bf16 copy of the updated parameter (nullptr: none) — the
// compute-dtype weights the next forward reads, refreshed here instead of by per-step casts.
// omb1 / omb2: the (1 - beta) weights of lerp / addcmul (torch computes them in f64 from its Python
// floats; the guarded entry point does the same).
// finite (optional, device): 0 = the loss guard fired (loss.py:190-198) — nothing is updated, as
// when the reference's step sees no grad.
// steps_in / steps_out (optional, device f32 per tensor): the step counts before / after this
// update. With them bc1 / bc2 come from steps_in[t] + 1 in f64 (what the host computes from its
// counter), and a skipped (finite = 0) update leaves the count where it was, so the NEXT update's
// bias correction is the one torch.optim.AdamW uses when that step never happened. The count is
// written to a second buffer (block 0 of the tensor) so that no block reads a count another
// block has already advanced; the caller swaps the two buffers.
// One element of the update. Contraction off: the two launch forms below (and any vector width)
// round identically, whatever the surrounding code lets the backend fuse.
IVIT_DEV void adamw_elem(float gi, float& pi, float& mi, float& vi, float keep, float omb1, float b2, float omb2,
                         float bc2s, float eps, float step) {
#pragma clang fp contract(off)
  pi = pi * keep;
  mi = mi + omb1 * (gi - mi);
  vi = vi * b2 + omb2 * gi * gi;
  const float den = sqrtf(vi) / bc2s + eps;
  pi = pi - step * (mi / den);
}

__global__ __launch_bounds__(256) void adamw_kernel(void* const* params, void* const* grads, void* const* ms,
                                                    void* const* vs, const long* sizes, float lr, float b1, float b2,
                                                    float eps, float wd, float bc1, float bc2s, void* const* shadows,
                                                    int sstride, const float* finite, const float* steps_in,
                                                    float* steps_out, double b1d, double b2d, float omb1,
                                                    float omb2) {
  const int t = blockIdx.y;
  const bool go = finite == nullptr || *finite != 0.f;
  const long n = sizes[t];
  if (steps_in != nullptr) {
    const float s0 = steps_in[t];
    if (blockIdx.x == 0 && threadIdx.x == 0) steps_out[t] = go ? s0 + 1.f : s0;
    // the grid is sized for the largest tensor: most blocks of a small one have no elements, and
    // must leave before the f64 pow (it made the launch 4x slower)
    if (!go || (long)blockIdx.x * blockDim.x >= n) return;
    const double s = (double)s0 + 1.0;
    bc1 = (float)(1.0 - pow(b1d, s));
    bc2s = (float)sqrt(1.0 - pow(b2d, s));
  }
  if (!go) return;
  float* p = (float*)params[t];
  const float* g = (const float*)grads[t];
  float* m = (float*)ms[t];
  float* v = (float*)vs[t];
  bf16* sh = shadows ? (bf16*)shadows[(long)sstride * t] : nullptr;
  const float step = lr / bc1, keep = 1.f - lr * wd;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float pi = p[i], mi = m[i], vi = v[i];
    adamw_elem(g[i], pi, mi, vi, keep, omb1, b2, omb2, bc2s, eps, step);
    p[i] = pi;
    m[i] = mi;
    v[i] = vi;
    if (sh) sh[i] = (bf16)pi;
  }
}

// The same update over a flat list of fixed-size chunks (ivit_adamw_chunked): one workgroup per
// chunk of AW_CHUNK elements of one tensor (chunks[b] = (tensor, chunk index)), 16-B accesses where
// the tensor's four arrays allow them. The 2D form above launches max_size / 256 workgroups for EVERY
// tensor (335 k for IntentNetViT's 327 parameters, nearly all of them leaving at once), which kept
// the update at ~3.7 TB/s; this grid has exactly the ~15.7 k chunks there are. Same element update
// (adamw_elem): bit-identical results.
// SCALED (ivit_adamw_chunked_scaled): every gradient element is first multiplied by *grad_scale (the
// clip coefficient of ivit_grad_norm) — the product ivit_grad_scale would have stored, so the fused and
// the unfused form give the same bits. The unscaled instantiation is the kernel as it was.
// EMA (ivit_adamw_chunked_ema): emas[t] (f32, null per tensor = not averaged) is the tensor's
// exponential moving average, moved towards the parameter this launch has just computed and still
// holds in a register: e += omd * (p_new - e), three f32 operations with contraction off, so a host
// that repeats them on the stored weights gets the same bits. omd = (float)(1 - d) with d in f64,
// formed once per workgroup before the element loop: d = ema_decay, or under ema_warmup
// min(ema_decay, (1 + n) / (10 + n)) with n = steps_in[t] + 1, this tensor's count after the update
// (device counts only: without them the host knows n and passes the step's d as ema_decay). It sits
// behind the finite exit like the pow of the bias corrections, so a skipped launch pays for neither
// and leaves e alone. The EMA = false instantiations are the kernels as they were.
// PT (ivit_adamw_chunked_pt): hyper[t] = (lr_scale, weight_decay) of tensor t, a device f32 [n][2] table
// that lets parameter groups which differ only in those two share the launch (layer-wise lr decay, no
// decay on 1-D tensors). It is uniform over the workgroup and read once, before the element loop:
//   lr_t = lr * hyper[t].x ; keep = fma(-lr_t, hyper[t].y, 1) ; step = lr_t / bc1
// lr_t is the rounded f32 product a host forms for a per-group launch, and keep is the single-rounding
// form 1 - lr * wd has in the PT = false kernels (the backend contracts it there; written out here, so
// the table launch and a launch per group give the same bits). The scalar wd is not read. The
// PT = false instantiations are the kernels as they were.
constexpr int AW_CHUNK = 4096;
IVIT_DEV float scaled_grad(float g, float s) {
#pragma clang fp contract(off)
  return g * s;
}
IVIT_DEV float ema_elem(float e, float p, float omd) {
#pragma clang fp contract(off)
  const float diff = p - e;
  const float mv = omd * diff;
  return e + mv;
}
IVIT_DEV float scaled_lr(float lr, float s) {
#pragma clang fp contract(off)
  return lr * s;
}
template <bool SCALED, bool EMA, bool PT = false>
__global__ __launch_bounds__(256) void adamw_chunk_kernel(void* const* params, void* const* grads, void* const* ms,
                                                          void* const* vs, const long* sizes, const int2* chunks,
                                                          float lr, float b2, float eps, float wd, float bc1,
                                                          float bc2s, void* const* shadows, const float* finite,
                                                          const float* steps_in, float* steps_out, double b1d,
                                                          double b2d, float omb1, float omb2,
                                                          const float* grad_scale, void* const* emas,
                                                          double ema_decay, int ema_warmup,
                                                          const float2* hyper = nullptr) {
  const int2 ck = chunks[blockIdx.x];
  const int t = ck.x;
  // PT: this tensor's (lr_scale, weight_decay), read ahead of the count store below so that it stays
  // a scalar load (uniform over the workgroup, once per workgroup)
  float2 hy = make_float2(1.f, 0.f);
  if constexpr (PT) hy = hyper[t];
  const bool go = finite == nullptr || *finite != 0.f;
  double nstep = 0.0;  // EMA: the count after this update (device counts)
  if (steps_in != nullptr) {
    const float s0 = steps_in[t];
    if (ck.y == 0 && threadIdx.x == 0) steps_out[t] = go ? s0 + 1.f : s0;
    if (!go) return;
    const double s = (double)s0 + 1.0;
    bc1 = (float)(1.0 - pow(b1d, s));
    bc2s = (float)sqrt(1.0 - pow(b2d, s));
    nstep = s;
  }
  if (!go) return;
  float omd = 0.f;
  if constexpr (EMA) {
    double d = ema_decay;
    if (ema_warmup) {
      const double w = (1.0 + nstep) / (10.0 + nstep);
      d = w < d ? w : d;
    }
    omd = (float)(1.0 - d);
  }
  const long off = (long)ck.y * AW_CHUNK;
  const long n = sizes[t];
  const int len = (int)min((long)AW_CHUNK, n - off);
  float* p = (float*)params[t] + off;
  const float* g = (const float*)grads[t] + off;
  float* m = (float*)ms[t] + off;
  float* v = (float*)vs[t] + off;
  bf16* sh = shadows && shadows[t] ? (bf16*)shadows[t] + off : nullptr;
  float* ea = nullptr;
  if constexpr (EMA) ea = emas[t] ? (float*)emas[t] + off : nullptr;
  float step, keep;
  if constexpr (PT) {
    const float lrt = scaled_lr(lr, hy.x);
    keep = __builtin_fmaf(-lrt, hy.y, 1.f);
    step = lrt / bc1;
  } else {
    step = lr / bc1, keep = 1.f - lr * wd;
  }
  float gs = 1.f;
  if constexpr (SCALED) gs = *grad_scale;
  auto upd = [&](float gi, float& pi, float& mi, float& vi) {
    if constexpr (SCALED) gi = scaled_grad(gi, gs);
    adamw_elem(gi, pi, mi, vi, keep, omb1, b2, omb2, bc2s, eps, step);
  };
  const bool vec = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0) &&
                   (((uintptr_t)sh & 7) == 0) && (((uintptr_t)ea & 15) == 0) && (len & 3) == 0;
  if (vec) {
    for (int i = threadIdx.x * 4; i < len; i += 1024) {
      const float4 gi = *(const float4*)(g + i);
      float4 pi = *(const float4*)(p + i), mi = *(const float4*)(m + i), vi = *(const float4*)(v + i);
      upd(gi.x, pi.x, mi.x, vi.x);
      upd(gi.y, pi.y, mi.y, vi.y);
      upd(gi.z, pi.z, mi.z, vi.z);
      upd(gi.w, pi.w, mi.w, vi.w);
      *(float4*)(p + i) = pi;
      *(float4*)(m + i) = mi;
      *(float4*)(v + i) = vi;
      if (sh) *(uint2*)(sh + i) = make_uint2(pk_bf16(pi.x, pi.y), pk_bf16(pi.z, pi.w));
      if constexpr (EMA) {
        if (ea) {
          float4 ei = *(const float4*)(ea + i);
          ei.x = ema_elem(ei.x, pi.x, omd);
          ei.y = ema_elem(ei.y, pi.y, omd);
          ei.z = ema_elem(ei.z, pi.z, omd);
          ei.w = ema_elem(ei.w, pi.w, omd);
          *(float4*)(ea + i) = ei;
        }
      }
    }
  } else {
    for (int i = threadIdx.x; i < len; i += 256) {
      float pi = p[i], mi = m[i], vi = v[i];
      upd(g[i], pi, mi, vi);
      p[i] = pi;
      m[i] = mi;
      v[i] = vi;
      if (sh) sh[i] = (bf16)pi;
      if constexpr (EMA) {
        if (ea) ea[i] = ema_elem(ea[i], pi, omd);
      }
    }
  }
}

// a[t] <-> b[t] element by element over the chunk grid (ivit_swap_chunked), each element read into a
// register and written to the other side: no third buffer. shadows[t] (bf16, null = none) receives
// the new a, as the update launch writes the new parameter. Same vector / scalar split.
__global__ __launch_bounds__(256) void swap_chunk_kernel(void* const* as, void* const* bs, const long* sizes,
                                                         const int2* chunks, void* const* shadows) {
  const int2 ck = chunks[blockIdx.x];
  const int t = ck.x;
  const long off = (long)ck.y * AW_CHUNK;
  const int len = (int)min((long)AW_CHUNK, sizes[t] - off);
  float* a = (float*)as[t] + off;
  float* b = (float*)bs[t] + off;
  bf16* sh = shadows && shadows[t] ? (bf16*)shadows[t] + off : nullptr;
  const bool vec = ((((uintptr_t)a | (uintptr_t)b) & 15) == 0) && (((uintptr_t)sh & 7) == 0) && (len & 3) == 0;
  if (vec) {
    for (int i = threadIdx.x * 4; i < len; i += 1024) {
      const float4 ai = *(const float4*)(a + i), bi = *(const float4*)(b + i);
      *(float4*)(a + i) = bi;
      *(float4*)(b + i) = ai;
      if (sh) *(uint2*)(sh + i) = make_uint2(pk_bf16(bi.x, bi.y), pk_bf16(bi.z, bi.w));
    }
  } else {
    for (int i = threadIdx.x; i < len; i += 256) {
      const float ai = a[i], bi = b[i];
      a[i] = bi;
      b[i] = ai;
      if (sh) sh[i] = (bf16)bi;
    }
  }
}

// ---- global gradient norm (ivit_grad_norm) ----
// Sum of a per-thread f64 value over the NW waves of the workgroup, in one fixed order: xor
// butterfly inside each wave (every lane ends with the same bits: IEEE addition commutes), then
// waves 0 .. NW-1 in order. Valid in thread 0.
template <int NW>
IVIT_DEV double block_sum_f64(double v, double* red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) t += red[w];
  return t;
}

// Pass 1: one workgroup per chunk. Thread t owns elements 4t .. 4t+3 (+1024k) of the chunk and adds
// their squares to its f64 sum in index order; the ownership and the order of every add are the
// same whether the four floats come from one 16-B load or from four 4-B loads (a chunk that is not
// 16-B aligned, or its ragged end), so the partial does not depend on where the tensor lies. The
// square of an f32 is exact in f64 (48 significant bits) and neither overflows nor underflows.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(void* const* grads, const long* sizes, const int2* chunks,
                                                         double* part) {
  __shared__ double red[4];
  const int2 ck = chunks[blockIdx.x];
  const long off = (long)ck.y * AW_CHUNK;
  const int len = (int)min((long)AW_CHUNK, sizes[ck.x] - off);
  const float* g = (const float*)grads[ck.x] + off;
  const bool al = al16(g);
  float4 x[AW_CHUNK / 1024];
#pragma unroll
  for (int k = 0; k < AW_CHUNK / 1024; ++k) {
    const int i = threadIdx.x * 4 + k * 1024;
    if (al && i + 4 <= len) {
      x[k] = *(const float4*)(g + i);
    } else {
      x[k].x = i < len ? g[i] : 0.f;
      x[k].y = i + 1 < len ? g[i + 1] : 0.f;
      x[k].z = i + 2 < len ? g[i + 2] : 0.f;
      x[k].w = i + 3 < len ? g[i + 3] : 0.f;
    }
  }
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < AW_CHUNK / 1024; ++k) {
    const double a = x[k].x, b = x[k].y, c = x[k].z, d = x[k].w;
    s += a * a;  // exact products: fused or not, the same bits
    s += b * b;
    s += c * c;
    s += d * d;
  }
  s = block_sum_f64<4>(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// Pass 2: one workgroup of GN_FINAL threads. Thread t adds partials t, t + GN_FINAL, ... in order
// (loaded eight at a time: a load per add would serialise ~15 L2 round trips), then the same
// workgroup sum; thread 0 writes the record {norm, coef, finite, 0} (clip_grad_norm_'s formula and
// clamp in f32) and updates the optional f64 stats {calls, clipped, non-finite, sum, max of finite
// norms}.
constexpr int GN_FINAL = 1024;
__global__ __launch_bounds__(GN_FINAL) void grad_norm_final_kernel(const double* part, int n, float max_norm,
                                                                   const float* finite_in, float* result,
                                                                   double* stats) {
#pragma clang fp contract(off)
  __shared__ double red[GN_FINAL / 64];
  double s = 0.0;
  for (int i0 = threadIdx.x; i0 < n; i0 += 8 * GN_FINAL) {
    double v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int i = i0 + k * GN_FINAL;
      v[k] = i < n ? part[i] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) s += v[k];  // + 0.0 past the end: the bits of a sum of squares stay
  }
  s = block_sum_f64<GN_FINAL / 64>(s, red);
  if (threadIdx.x != 0) return;
  const float norm = (float)sqrt(s);
  const bool nf = isfinite(norm);
  const float q = max_norm / (norm + 1e-6f);
  const float coef = nf ? (q < 1.f ? q : 1.f) : 1.f;
  result[0] = norm;
  result[1] = coef;
  result[2] = ((finite_in == nullptr || *finite_in != 0.f) && nf) ? 1.f : 0.f;
  result[3] = 0.f;
  if (stats != nullptr) {
    stats[0] += 1.0;
    if (coef < 1.f) stats[1] += 1.0;
    if (!nf) stats[2] += 1.0;
    if (nf) {
      stats[3] += (double)norm;
      if ((double)norm > stats[4]) stats[4] = (double)norm;
    }
  }
}

// g *= *coef over the chunk grid (the second half of clip_grad_norm_). The products are the ones
// adamw_chunk_kernel<SCALED = true> forms in registers. coef == 1 (no clipping) would rewrite every element
// with itself: nothing is stored.
__global__ __launch_bounds__(256) void grad_scale_kernel(void* const* grads, const long* sizes, const int2* chunks,
                                                         const float* coef) {
  const float c = *coef;
  if (c == 1.f) return;
  const int2 ck = chunks[blockIdx.x];
  const long off = (long)ck.y * AW_CHUNK;
  const int len = (int)min((long)AW_CHUNK, sizes[ck.x] - off);
  float* g = (float*)grads[ck.x] + off;
  if (al16(g) && (len & 3) == 0) {
    for (int i = threadIdx.x * 4; i < len; i += 1024) {
      float4 v = *(const float4*)(g + i);
      v.x = scaled_grad(v.x, c);
      v.y = scaled_grad(v.y, c);
      v.z = scaled_grad(v.z, c);
      v.w = scaled_grad(v.w, c);
      *(float4*)(g + i) = v;
    }
  } else {
    for (int i = threadIdx.x; i < len; i += 256) g[i] = scaled_grad(g[i], c);
  }
}

}  // namespace

extern "C" int ivit_cast(const void* x, int x_dtype, void* y, int y_dtype, long n, void* stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(cast_kernel, dim3(ivit_cdiv(n, 256)), dim3(256), 0, ivit_stream(stream), x, x_dtype, y, y_dtype,
                     n);
  IVIT_LAUNCH_CHECK();
  return 0;
}

extern "C" int ivit_add_act_grad(const void* a, int a_dtype, const void* b, int b_dtype, const void* pre,
                                 int pre_dtype, const float* row_scale, long row_elems, void* out, int out_dtype, long n,
                                 void* stream) {
  if (n <= 0) return 0;
  const long re = row_elems > 0 ? row_elems : 1;
  if (n % 8 == 0 && (!row_scale || re % 8 == 0) && hal16(a) && (!b || hal16(b)) && (!pre || hal16(pre)) && hal16(out))
    hipLaunchKernelGGL(add_act_grad8_kernel, dim3(ivit_cdiv(n / 8, 256)), dim3(256), 0, ivit_stream(stream), a, a_dtype,
                       b, b_dtype, pre, pre_dtype, row_scale, re, out, out_dtype, n);
  else
    hipLaunchKernelGGL(add_act_grad_kernel, dim3(ivit_cdiv(n, 256)), dim3(256), 0, ivit_stream(stream), a, a_dtype, b,
                       b_dtype, pre, pre_dtype, row_scale, re, out, out_dtype, n);
  IVIT_LAUNCH_CHECK();
  return 0;
}

extern "C" int ivit_copy_cols(const void* src, long lds, void* dst, long ldd, long rows, long cols, int dtype,
                              void* stream) {
  if (rows * cols <= 0) return 0;
  hipLaunchKernelGGL(copy_cols_kernel, dim3(ivit_cdiv(rows * cols, 256)), dim3(256), 0, ivit_stream(stream), src, lds,
                     dst, ldd, rows, cols, dtype);
  IVIT_LAUNCH_CHECK();
  return 0;
}

extern "C" int ivit_split_heads(const float* h, long ldh, long M, long A, long K, float* cls, float* box,
                                float* intent, void* stream) {
  IVIT_CHECK_ARG(ldh >= A * 7 + A * K, "ivit_split_heads: ldh too small");
  if (M <= 0) return 0;
  hipLaunchKernelGGL(split_heads_kernel, dim3(ivit_cdiv(M * A, 256)), dim3(256), 0, ivit_stream(stream), h, ldh, M,
                     (int)A, (int)K, cls, box, intent);
  IVIT_LAUNCH_CHECK();
  return 0;
}

extern "C" int ivit_merge_heads_grad(const float* dcls, const float* dbox, const float* dint, long M, long A, long K,
                                     void* dh, long ldh, int dh_dtype, void* stream) {
  if (M <= 0) return 0;
  hipLaunchKernelGGL(merge_heads_kernel, dim3(ivit_cdiv(M * ldh, 256)), dim3(256), 0, ivit_stream(stream), dcls, dbox,
                     dint, M, (int)A, (int)K, dh, ldh, dh_dtype);
  IVIT_LAUNCH_CHECK();
  return 0;
}

extern "C" int ivit_adamw(long n_tensors, void* const* params, void* const* grads, void* const* exp_avg,
                          void* const* exp_avg_sq, const long* sizes, long max_size, float lr, float beta1,
                          float beta2, float eps, float weight_decay, float bc1, float bc2_sqrt, void* stream) {
  if (n_tensors <= 0) return 0;
  IVIT_CHECK_ARG(n_tensors < 65536, "ivit_adamw: too many tensors");
  int gx = ivit_cdiv(max_size, 256);
  if (gx > 1024) gx = 1024;
  hipLaunchKernelGGL(adamw_kernel, dim3(gx, n_tensors), dim3(256), 0, ivit_stream(stream), params, grads, exp_avg,
                     exp_avg_sq, sizes, lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, (void* const*)nullptr, 1,
                     (const float*)nullptr, (const float*)nullptr, (float*)nullptr, 0.0, 0.0, 1.f - beta1, 1.f - beta2);
  IVIT_LAUNCH_CHECK();
  return 0;
}

extern "C" int ivit_adamw_shadow(long n_tensors, void* const* params, void* const* grads, void* const* exp_avg,
                                 void* const* exp_avg_sq, void* const* shadows, const long* sizes, long max_size,
                                 float lr, float beta1, float beta2, float eps, float weight_decay, float bc1,
                                 float bc2_sqrt, void* stream) {
  if (n_tensors <= 0) return 0;
  IVIT_CHECK_ARG(n_tensors < 65536, "ivit_adamw_shadow: too many tensors");
  IVIT_CHECK_ARG(shadows != nullptr, "ivit_adamw_shadow: shadow table is null");
  int gx = ivit_cdiv(max_size, 256);
  if (gx > 1024) gx = 1024;
  hipLaunchKernelGGL(adamw_kernel, dim3(gx, n_tensors), dim3(256), 0, ivit_stream(stream), params, grads, exp_avg,
                     exp_avg_sq, sizes, lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, shadows, 1,
                     (const float*)nullptr, (const float*)nullptr, (float*)nullptr, 0.0, 0.0, 1.f - beta1, 1.f - beta2);
  IVIT_LAUNCH_CHECK();
  return 0;
}

extern "C" int ivit_adamw_guarded(long n_tensors, void* const* params, void* const* grads, void* const* exp_avg,
                                  void* const* exp_avg_sq, void* const* shadows, const long* sizes, long max_size,
                                  float lr, double beta1, double beta2, float eps, float weight_decay, float bc1,
                                  float bc2_sqrt, const float* finite, const float* steps_in, float* steps_out,
                                  void* stream) {
  if (n_tensors <= 0) return 0;
  IVIT_CHECK_ARG(n_tensors < 65536, "ivit_adamw_guarded: too many tensors");
  IVIT_CHECK_ARG((steps_in == nullptr) == (steps_out == nullptr), "ivit_adamw_guarded: steps_in / steps_out pair");
  IVIT_CHECK_ARG(steps_in == nullptr || steps_in != steps_out, "ivit_adamw_guarded: steps_out aliases steps_in");
  int gx = ivit_cdiv(max_size, 256);
  if (gx > 1024) gx = 1024;
  hipLaunchKernelGGL(adamw_kernel, dim3(gx, n_tensors), dim3(256), 0, ivit_stream(stream), params, grads, exp_avg,
                     exp_avg_sq, sizes, lr, (float)beta1, (float)beta2, eps, weight_decay, bc1, bc2_sqrt, shadows, 1,
                     finite, steps_in, steps_out, beta1, beta2, (float)(1.0 - beta1), (float)(1.0 - beta2));
  IVIT_LAUNCH_CHECK();
  return 0;
}

extern "C" long ivit_adamw_chunk_elems() { return AW_CHUNK; }

extern "C" int ivit_adamw_chunked(long n_tensors, void* const* params, void* const* grads, void* const* exp_avg,
                                  void* const* exp_avg_sq, void* const* shadows, const long* sizes,
                                  const int* chunks, long n_chunks, float lr, double beta1, double beta2, float eps,
                                  float weight_decay, float bc1, float bc2_sqrt, const float* finite,
                                  const float* steps_in, float* steps_out, void* stream) {
  if (n_tensors <= 0 || n_chunks <= 0) return 0;
  IVIT_CHECK_ARG(chunks != nullptr && n_chunks < (1L << 31), "ivit_adamw_chunked: bad chunk table");
  IVIT_CHECK_ARG((steps_in == nullptr) == (steps_out == nullptr), "ivit_adamw_chunked: steps_in / steps_out pair");
  IVIT_CHECK_ARG(steps_in == nullptr || steps_in != steps_out, "ivit_adamw_chunked: steps_out aliases steps_in");
  IVIT_CHECK_ARG(((uintptr_t)chunks & 7) == 0, "ivit_adamw_chunked: misaligned chunk table");
  hipLaunchKernelGGL((adamw_chunk_kernel<false, false>), dim3((unsigned)n_chunks), dim3(256), 0, ivit_stream(stream),
                     params, grads, exp_avg, exp_avg_sq, sizes, (const int2*)chunks, lr, (float)beta2, eps,
                     weight_decay, bc1, bc2_sqrt, shadows, finite, steps_in, steps_out, beta1, beta2,
                     (float)(1.0 - beta1), (float)(1.0 - beta2), (const float*)nullptr, (void* const*)nullptr, 0.0, 0);
  IVIT_LAUNCH_CHECK();
  return 0;
}

extern "C" int ivit_adamw_chunked_scaled(long n_tensors, void* const* params, void* const* grads,
                                         void* const* exp_avg, void* const* exp_avg_sq, void* const* shadows,
                                         const long* sizes, const int* chunks, long n_chunks, float lr, double beta1,
                                         double beta2, float eps, float weight_decay, float bc1, float bc2_sqrt,
                                         const float* finite, const float* steps_in, float* steps_out,
                                         const float* grad_scale, void* stream) {
  if (grad_scale == nullptr)
    return ivit_adamw_chunked(n_tensors, params, grads, exp_avg, exp_avg_sq, shadows, sizes, chunks, n_chunks, lr,
                              beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, finite, steps_in, steps_out, stream);
  if (n_tensors <= 0 || n_chunks <= 0) return 0;
  IVIT_CHECK_ARG(chunks != nullptr && n_chunks < (1L << 31), "ivit_adamw_chunked_scaled: bad chunk table");
  IVIT_CHECK_ARG((steps_in == nullptr) == (steps_out == nullptr),
                 "ivit_adamw_chunked_scaled: steps_in / steps_out pair");
  IVIT_CHECK_ARG(steps_in == nullptr || steps_in != steps_out, "ivit_adamw_chunked_scaled: steps_out aliases steps_in");
  IVIT_CHECK_ARG(((uintptr_t)chunks & 7) == 0, "ivit_adamw_chunked_scaled: misaligned chunk table");
  hipLaunchKernelGGL((adamw_chunk_kernel<true, false>), dim3((unsigned)n_chunks), dim3(256), 0, ivit_stream(stream),
                     params, grads, exp_avg, exp_avg_sq, sizes, (const int2*)chunks, lr, (float)beta2, eps,
                     weight_decay, bc1, bc2_sqrt, shadows, finite, steps_in, steps_out, beta1, beta2,
                     (float)(1.0 - beta1), (float)(1.0 - beta2), grad_scale, (void* const*)nullptr, 0.0, 0);
  IVIT_LAUNCH_CHECK();
  return 0;
}

extern "C" int ivit_adamw_chunked_ema(long n_tensors, void* const* params, void* const* grads, void* const* exp_avg,
                                      void* const* exp_avg_sq, void* const* shadows, const long* sizes,
                                      const int* chunks, long n_chunks, float lr, double beta1, double beta2,
                                      float eps, float weight_decay, float bc1, float bc2_sqrt, const float* finite,
                                      const float* steps_in, float* steps_out, const float* grad_scale,
                                      void* const* emas, double ema_decay, int ema_warmup, void* stream) {
  if (emas == nullptr)
    return ivit_adamw_chunked_scaled(n_tensors, params, grads, exp_avg, exp_avg_sq, shadows, sizes, chunks, n_chunks,
                                     lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, finite, steps_in, steps_out,
                                     grad_scale, stream);
  IVIT_CHECK_ARG(ema_decay >= 0.0 && ema_decay < 1.0, "ivit_adamw_chunked_ema: ema_decay must be in [0, 1) (got %g)",
                 ema_decay);  // NaN fails too
  IVIT_CHECK_ARG(!ema_warmup || steps_in != nullptr,
                 "ivit_adamw_chunked_ema: ema_warmup needs the device step counts (without steps_in the host "
                 "passes the step's decay as ema_decay)");
  IVIT_CHECK_ARG(((uintptr_t)emas & 7) == 0, "ivit_adamw_chunked_ema: misaligned ema table");
  if (n_tensors <= 0 || n_chunks <= 0) return 0;
  IVIT_CHECK_ARG(chunks != nullptr && n_chunks < (1L << 31), "ivit_adamw_chunked_ema: bad chunk table");
  IVIT_CHECK_ARG((steps_in == nullptr) == (steps_out == nullptr), "ivit_adamw_chunked_ema: steps_in / steps_out pair");
  IVIT_CHECK_ARG(steps_in == nullptr || steps_in != steps_out, "ivit_adamw_chunked_ema: steps_out aliases steps_in");
  IVIT_CHECK_ARG(((uintptr_t)chunks & 7) == 0, "ivit_adamw_chunked_ema: misaligned chunk table");
  const dim3 grid((unsigned)n_chunks), block(256);
  if (grad_scale != nullptr)
    hipLaunchKernelGGL((adamw_chunk_kernel<true, true>), grid, block, 0, ivit_stream(stream), params, grads, exp_avg,
                       exp_avg_sq, sizes, (const int2*)chunks, lr, (float)beta2, eps, weight_decay, bc1, bc2_sqrt,
                       shadows, finite, steps_in, steps_out, beta1, beta2, (float)(1.0 - beta1), (float)(1.0 - beta2),
                       grad_scale, emas, ema_decay, ema_warmup);
  else
    hipLaunchKernelGGL((adamw_chunk_kernel<false, true>), grid, block, 0, ivit_stream(stream), params, grads, exp_avg,
                       exp_avg_sq, sizes, (const int2*)chunks, lr, (float)beta2, eps, weight_decay, bc1, bc2_sqrt,
                       shadows, finite, steps_in, steps_out, beta1, beta2, (float)(1.0 - beta1), (float)(1.0 - beta2),
                       (const float*)nullptr, emas, ema_decay, ema_warmup);
  IVIT_LAUNCH_CHECK();
  return 0;
}

extern "C" int ivit_adamw_chunked_pt(long n_tensors, void* const* params, void* const* grads, void* const* exp_avg,
                                     void* const* exp_avg_sq, void* const* shadows, const long* sizes,
                                     const int* chunks, long n_chunks, float lr, double beta1, double beta2,
                                     float eps, float weight_decay, float bc1, float bc2_sqrt, const float* finite,
                                     const float* steps_in, float* steps_out, const float* grad_scale,
                                     void* const* emas, double ema_decay, int ema_warmup, const float* hyper,
                                     void* stream) {
  if (hyper == nullptr)
    return ivit_adamw_chunked_ema(n_tensors, params, grads, exp_avg, exp_avg_sq, shadows, sizes, chunks, n_chunks, lr,
                                  beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, finite, steps_in, steps_out,
                                  grad_scale, emas, ema_decay, ema_warmup, stream);
  IVIT_CHECK_ARG(((uintptr_t)hyper & 7) == 0, "ivit_adamw_chunked_pt: misaligned hyper table");
  IVIT_CHECK_ARG(lr >= 0.f && __builtin_isfinite(lr), "ivit_adamw_chunked_pt: lr must be finite and >= 0 (got %g)",
                 (double)lr);  // NaN fails too
  if (emas != nullptr) {
    IVIT_CHECK_ARG(ema_decay >= 0.0 && ema_decay < 1.0, "ivit_adamw_chunked_pt: ema_decay must be in [0, 1) (got %g)",
                   ema_decay);  // NaN fails too
    IVIT_CHECK_ARG(!ema_warmup || steps_in != nullptr,
                   "ivit_adamw_chunked_pt: ema_warmup needs the device step counts (without steps_in the host "
                   "passes the step's decay as ema_decay)");
    IVIT_CHECK_ARG(((uintptr_t)emas & 7) == 0, "ivit_adamw_chunked_pt: misaligned ema table");
  }
  if (n_tensors <= 0 || n_chunks <= 0) return 0;
  IVIT_CHECK_ARG(chunks != nullptr && n_chunks < (1L << 31), "ivit_adamw_chunked_pt: bad chunk table");
  IVIT_CHECK_ARG((steps_in == nullptr) == (steps_out == nullptr), "ivit_adamw_chunked_pt: steps_in / steps_out pair");
  IVIT_CHECK_ARG(steps_in == nullptr || steps_in != steps_out, "ivit_adamw_chunked_pt: steps_out aliases steps_in");
  IVIT_CHECK_ARG(((uintptr_t)chunks & 7) == 0, "ivit_adamw_chunked_pt: misaligned chunk table");
  const dim3 grid((unsigned)n_chunks), block(256);
#define IVIT_AW_PT(S, E)                                                                                              \
  hipLaunchKernelGGL((adamw_chunk_kernel<S, E, true>), grid, block, 0, ivit_stream(stream), params, grads, exp_avg,   \
                     exp_avg_sq, sizes, (const int2*)chunks, lr, (float)beta2, eps, weight_decay, bc1, bc2_sqrt,      \
                     shadows, finite, steps_in, steps_out, beta1, beta2, (float)(1.0 - beta1), (float)(1.0 - beta2),  \
                     grad_scale, emas, ema_decay, ema_warmup, (const float2*)hyper)
  if (grad_scale != nullptr && emas != nullptr)
    IVIT_AW_PT(true, true);
  else if (grad_scale != nullptr)
    IVIT_AW_PT(true, false);
  else if (emas != nullptr)
    IVIT_AW_PT(false, true);
  else
    IVIT_AW_PT(false, false);
#undef IVIT_AW_PT
  IVIT_LAUNCH_CHECK();
  return 0;
}

extern "C" int ivit_swap_chunked(long n_tensors, void* const* a, void* const* b, const long* sizes, const int* chunks,
                                 long n_chunks, void* const* shadows, void* stream) {
  if (n_tensors <= 0 || n_chunks <= 0) return 0;
  IVIT_CHECK_ARG(a != nullptr && b != nullptr && sizes != nullptr, "ivit_swap_chunked: null tensor tables");
  IVIT_CHECK_ARG(chunks != nullptr && n_chunks < (1L << 31), "ivit_swap_chunked: bad chunk table");
  IVIT_CHECK_ARG(((uintptr_t)chunks & 7) == 0, "ivit_swap_chunked: misaligned chunk table");
  hipLaunchKernelGGL(swap_chunk_kernel, dim3((unsigned)n_chunks), dim3(256), 0, ivit_stream(stream), a, b, sizes,
                     (const int2*)chunks, shadows);
  IVIT_LAUNCH_CHECK();
  return 0;
}

extern "C" long ivit_grad_norm_workspace(long n_chunks) { return (n_chunks > 0 ? n_chunks : 1) * (long)sizeof(double); }

extern "C" int ivit_grad_norm(long n_tensors, void* const* grads, const long* sizes, const int* chunks, long n_chunks,
                              float max_norm, const float* finite_in, void* workspace, long workspace_bytes,
                              float* result, double* stats, void* stream) {
  IVIT_CHECK_ARG(max_norm > 0.f, "ivit_grad_norm: max_norm must be > 0 (got %g)", (double)max_norm);  // NaN fails too
  IVIT_CHECK_ARG(n_tensors >= 0 && n_chunks >= 0 && n_chunks < (1L << 31), "ivit_grad_norm: bad counts");
  IVIT_CHECK_ARG(n_tensors == 0 || (grads != nullptr && sizes != nullptr), "ivit_grad_norm: null tensor tables");
  IVIT_CHECK_ARG(n_chunks == 0 || (n_tensors > 0 && chunks != nullptr), "ivit_grad_norm: null chunk table");
  IVIT_CHECK_ARG(((uintptr_t)chunks & 7) == 0, "ivit_grad_norm: misaligned chunk table");
  IVIT_CHECK_ARG(result != nullptr, "ivit_grad_norm: result is null");
  IVIT_CHECK_ARG(workspace != nullptr && ((uintptr_t)workspace & 7) == 0 &&
                     workspace_bytes >= ivit_grad_norm_workspace(n_chunks),
                 "ivit_grad_norm: workspace too small or misaligned (%ld bytes, need %ld)", workspace_bytes,
                 ivit_grad_norm_workspace(n_chunks));
  IVIT_CHECK_ARG(((uintptr_t)stats & 7) == 0, "ivit_grad_norm: misaligned stats");
  if (n_chunks > 0) {
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)n_chunks), dim3(256), 0, ivit_stream(stream), grads, sizes,
                       (const int2*)chunks, (double*)workspace);
    IVIT_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(GN_FINAL), 0, ivit_stream(stream), (const double*)workspace,
                     (int)n_chunks, max_norm, finite_in, result, stats);
  IVIT_LAUNCH_CHECK();
  return 0;
}

extern "C" int ivit_grad_scale(long n_tensors, void* const* grads, const long* sizes, const int* chunks, long n_chunks,
                               const float* coef, void* stream) {
  if (n_tensors <= 0 || n_chunks <= 0) return 0;
  IVIT_CHECK_ARG(grads != nullptr && sizes != nullptr, "ivit_grad_scale: null tensor tables");
  IVIT_CHECK_ARG(chunks != nullptr && n_chunks < (1L << 31), "ivit_grad_scale: bad chunk table");
  IVIT_CHECK_ARG(((uintptr_t)chunks & 7) == 0, "ivit_grad_scale: misaligned chunk table");
  IVIT_CHECK_ARG(coef != nullptr, "ivit_grad_scale: coef is null");
  hipLaunchKernelGGL(grad_scale_kernel, dim3((unsigned)n_chunks), dim3(256), 0, ivit_stream(stream), grads, sizes,
                     (const int2*)chunks, coef);
  IVIT_LAUNCH_CHECK();
  return 0;
}

extern "C" int ivit_act_fwd(int act, const void* x, int x_dtype, void* y, int y_dtype, long n, void* stream) {
  IVIT_CHECK_ARG(act == IVIT_ACT_GELU || act == IVIT_ACT_RELU || act == IVIT_ACT_NONE, "ivit_act_fwd: bad act %d", act);
  if (n <= 0) return 0;
  hipLaunchKernelGGL(act_fwd_kernel, dim3(ivit_cdiv(n, 256)), dim3(256), 0, ivit_stream(stream), act, x, x_dtype, y,
                     y_dtype, n);
  IVIT_LAUNCH_CHECK();
  return 0;
}

extern "C" int ivit_act_bwd(int act, const void* dy, int dy_dtype, const void* x, int x_dtype, void* dx, int dx_dtype,
                            long n, void* stream) {
  IVIT_CHECK_ARG(act == IVIT_ACT_GELU || act == IVIT_ACT_RELU || act == IVIT_ACT_NONE, "ivit_act_bwd: bad act %d", act);
  if (n <= 0) return 0;
  hipLaunchKernelGGL(act_bwd_kernel, dim3(ivit_cdiv(n, 256)), dim3(256), 0, ivit_stream(stream), act, dy, dy_dtype, x,
                     x_dtype, dx, dx_dtype, n);
  IVIT_LAUNCH_CHECK();
  return 0;
}
